"""Exact-arithmetic ("integer") nets for the tower tests: every folded weight, shift, activation and logit is an integer
(the value head a dyadic fraction), every product and partial sum exact in f32 in any summation order.  On such a net
the towers' accumulation order does not matter, so a tower in any dtype must equal oracle.net_oracle.forward_lowp bit for
bit; a structural or rounding defect shows as an exact mismatch instead of hiding in a tolerance.

make_net(blocks, filters, features, fmt, seed) draws the net for the boards it will be run on and calibrates it layer by
layer in the emulator (sparse small-integer weights, batch-norm means at per-channel percentiles of those boards), so
that activations stay alive and bounded; check_preconditions asserts on exactly those boards what the tests rely on."""
import functools

import numpy as np

from oracle import net_oracle

EXACT = 2 ** 24                     # integers below this are exact in f32
# dyadic batch-norm scales float(1/sqrt(var + eps)) and a float32 variance that gives each one exactly
# (the double inv is within 2e-8 of it, so float(-mean * inv) is exactly -mean * scale for the means drawn here)
VAR_FOR_SCALE = {1.0: np.float32(0.999), 0.75: np.float32(1.7767777), 1.5: np.float32(0.44344443),
                 0.5: np.float32(3.999), 0.25: np.float32(15.999)}
# the raw weight is a multiple of MULT[s] so that the folded weight raw * s is an integer
MULT = {1.0: 1, 0.75: 4, 1.5: 2, 0.5: 2, 0.25: 4}
# activation range the calibration aims for: enough above 256 (bf16) / 2048 (f16) to round, below 2^15 for f16
LO = {"f32": 600, "bf16": 600, "f16": 3000}
HI = 20000


def _scales(rng, n, first):
    """mostly 1; the first layer (whose inputs are 0 / 1) carries the non-power-of-two scales that test the fold order"""
    p = [0.4, 0.3, 0.3, 0.0, 0.0] if first else [0.8, 0.03, 0.03, 0.07, 0.07]
    return rng.choice(list(VAR_FOR_SCALE), size=n, p=p)


def _shift_for(target, s):
    """(mean, shift) with shift = float(-mean * inv) an integer close to `target`"""
    step = 3 if s in (0.75, 1.5) else 1
    t = step * int(np.round(target / step))
    mean = np.float32(-t / s)
    assert mean == -t / s
    return mean, t


def _draw_first(rng, fmt, s):
    """raw weights (3,3,4) of one first-layer channel: a few small integers and one large weight that is not 16-bit
    representable before it is folded (its folded value is rounded, for s = 0.75 / 1.5 to another value than
    round(raw) * s)"""
    m = MULT[s]
    w = np.zeros((3, 3, 4), np.float32)
    idx = rng.choice(36, size=7, replace=False)
    vals = rng.integers(1, 120, size=7) * rng.choice([-1, 1], size=7)
    w.reshape(-1)[idx[:6]] = m * vals[:6]
    if fmt == "f16":
        k = 2 * int(rng.integers(1025, 1250)) + 1      # folded 3k-ish: > 2048 and odd, an f16 tie or inexact
    else:
        k = 2 * int(rng.integers(129, 400)) + 1        # > 256 and odd: not bf16
    w.reshape(-1)[idx[6]] = m * k * (1 if rng.random() < 0.7 else -1)
    if s == 1.0 and fmt != "f32":
        assert net_oracle._rounder(fmt)(w).tolist() != w.tolist()
    return w


def _draw_conv(rng, cin, s, amp, nnz, alive):
    """raw weights (3,3,cin) of one output channel: nnz entries of magnitude 1..amp (folded), inputs from live channels"""
    w = np.zeros((3, 3, cin), np.float32)
    m = MULT[s]
    for _ in range(nnz):
        i, j = rng.integers(0, 3, size=2)
        c = int(rng.choice(alive)) if len(alive) else int(rng.integers(0, cin))
        folded = int(rng.integers(1, amp + 1)) * (1 if rng.random() < 0.6 else -1)
        if s in (0.75, 1.5):
            w[i, j, c] += np.float32(m * folded)        # folded 3 * folded
        else:
            w[i, j, c] += np.float32(folded / s)
    return w


def _fold(w, s, fmt):
    return net_oracle._rounder(fmt)(w * np.float32(s)).astype(np.float64)


def _im2col(h):
    """(n,7,7,c) -> (n,7,7,9c), k index (i, j, c) as the weights (3,3,c) flatten"""
    n, c = h.shape[0], h.shape[3]
    hp = np.zeros((n, 9, 9, c))
    hp[:, 1:8, 1:8] = h
    return np.concatenate([hp[:, i:i + 7, j:j + 7] for i in range(3) for j in range(3)], axis=3)


def make_net(blocks, filters, features, fmt, seed, big_head=True):
    """-> (conv_weights, bn_params) in model.py's layout, calibrated on `features` (n,7,7,4) for dtype `fmt`.
    big_head=False leaves out the rounded large policy weights (logits then stay far enough below 2^24 / 8 for the
    symmetry average's f32 sum of eight logits to be exact)."""
    rng = np.random.default_rng(seed)
    rnd = net_oracle._rounder(fmt)
    lo = LO[fmt]
    h = np.asarray(features, np.float64)
    conv, bn = [], []
    block_in = t = None
    for layer in range(2 * blocks + 1):
        first = layer == 0
        second = layer > 0 and layer % 2 == 0          # a block's second conv: input t, residual block_in
        if layer % 2 == 1:
            block_in = h
        inp = t if second else h
        cin = inp.shape[3]
        cols = _im2col(inp)
        scales = _scales(rng, filters, first)
        alive = np.nonzero((inp > 0).mean(axis=(0, 1, 2)) > 0.05)[0]
        w = np.zeros((3, 3, cin, filters), np.float32)
        means = np.zeros(filters, np.float32)
        out = np.zeros(inp.shape[:3] + (filters,))
        for c in range(filters):
            s = float(scales[c])
            amp, nnz = 1, 2
            for attempt in range(40):
                wc = _draw_first(rng, fmt, s) if first else _draw_conv(rng, cin, s, amp, nnz, alive)
                fw = _fold(wc, s, fmt).reshape(-1)
                nz = np.nonzero(fw)[0]
                z = cols[..., nz] @ fw[nz]
                if second:
                    z = z + block_in[..., c]
                # shift: at a percentile of the channel, but low enough that the largest activation stays below HI
                target = -max(np.percentile(z, rng.uniform(35, 65)), z.max() - HI)
                mean, sh = _shift_for(target, s)
                a = np.maximum(rnd((z + sh).astype(np.float32)).astype(np.float64), 0)
                share = (a > 0).mean()
                if first or (a.max() >= lo and 0.15 <= share <= 0.9) or attempt == 39:
                    break
                if a.max() < lo:
                    amp, nnz = min(amp * 2, 64), min(nnz + 1, 4)
                else:
                    nnz = max(1, nnz - 1)
            w[..., c] = wc
            means[c] = mean
            out[..., c] = a
        conv.append(w)
        bn += [means, np.array([VAR_FOR_SCALE[float(s)] for s in scales], np.float32)]
        if layer % 2 == 1:
            t = out
        else:
            h = out
    # heads: sparse small integers on live channels (and, in bf16, one weight per logit channel that is rounded)
    alive = np.nonzero((h > 0).mean(axis=(0, 1, 2)) > 0.05)[0]
    if not len(alive):
        alive = np.arange(filters)
    hp = np.zeros((1, 1, filters, 17), np.float32)
    for o in range(17):
        for c in rng.choice(alive, size=4):
            hp[0, 0, c, o] += rng.integers(1, 10) * rng.choice([-1, 1])
        if fmt == "bf16" and big_head:
            hp[0, 0, rng.choice(alive), o] += 2 * rng.integers(128, 200) + 1
    hv = np.zeros((1, 1, filters, 1), np.float32)
    for c in rng.choice(alive, size=2, replace=False):
        hv[0, 0, c, 0] = rng.choice([-1, 1])
    vcell = (h @ rnd(hv[0, 0]).astype(np.float64))[..., 0].reshape(len(h), 49)
    j = (rng.integers(1, 4, size=49) * rng.choice([-1, 1], size=49)).astype(np.float64)
    top = max(np.abs(vcell * j).sum(axis=1).max(), 1.0)
    k = int(np.ceil(np.log2(top / 1.5)))              # sum |s| <= 1.5: tanh far from saturation
    fc_w = (j * 2.0 ** -k).astype(np.float32).reshape(49, 1)
    fc_b = np.array([rng.integers(-5, 6) * 2.0 ** -4], np.float32)
    conv += [hp, hv, fc_w, fc_b]
    return conv, bn


def _layer_trace(conv, bn, features, fmt):
    """per tower layer: (pre-rounding accumulator z, bound sum |w a| + |shift| + |residual|, activation out); and the
    tower's output"""
    layers = net_oracle.lowp_parameters(conv, bn, fmt)[0]
    rnd = net_oracle._rounder(fmt)
    h = np.asarray(features, np.float64)
    out, t = [], None
    for i, (w, shift) in enumerate(layers):
        w = w.astype(np.float64)
        second = i > 0 and i % 2 == 0
        inp = t if second else h
        z = net_oracle.conv2d_same(inp, w) + shift
        bound = net_oracle.conv2d_same(np.abs(inp), np.abs(w)) + np.abs(shift)
        if second:
            z, bound = z + h, bound + h
        a = np.maximum(rnd(z.astype(np.float32)).astype(np.float64), 0)
        out.append((z, bound, a))
        if i % 2 == 1:
            t = a
        else:
            h = a
    return out, h


def check_preconditions(conv, bn, features, fmt, sym=False, min_share=0.1, min_cell_share=0.02):
    """Assert, on exactly these boards, what makes the net an exact test of the `fmt` tower (sym: of the symmetry
    average, `features` then being all eight images of every board).  -> a dict of statistics."""
    rnd = net_oracle._rounder(fmt)
    layers, head_p, head_v, fc_w, fc_b = net_oracle.lowp_parameters(conv, bn, fmt)
    for w, shift in layers:
        assert (w == np.round(w)).all() and (shift == np.round(shift)).all(), "folded weights and shifts are integers"
    trace, h = _layer_trace(conv, bn, features, fmt)
    stats = {"layers": len(trace), "rounded": 0, "ties": 0, "values": 0}
    for i, (z, bound, a) in enumerate(trace):
        assert bound.max() < EXACT, ("layer %d: sum |w a| reaches 2^24" % i, bound.max())
        if fmt == "f16":
            assert a.max() < 2 ** 15, ("layer %d: f16 activation %g" % (i, a.max()))
        share = (a > 0).mean()
        assert share >= min_share, ("layer %d: %.3f of the activations are non-zero" % (i, share))
        cell_share = (a > 0).mean(axis=(0, 3)).min()
        assert cell_share >= min_cell_share, ("layer %d: a board cell has %.3f non-zero" % (i, cell_share))
        pos = z[z > 0].astype(np.float32)
        r = rnd(pos)
        stats["values"] += pos.size
        stats["rounded"] += int((r != pos).sum())
        if fmt != "f32":
            # exact ties: round to nearest even and truncation disagree on some of them
            below = net_oracle._truncate_bf16(pos) if fmt == "bf16" else net_oracle._truncate_f16(pos)
            if fmt == "bf16":
                above = (below.view(np.uint32) + np.uint32(0x10000)).view(np.float32)
            else:
                above = np.nextafter(below.astype(np.float16), np.float16(np.inf)).astype(np.float32)
            mid = (below.astype(np.float64) + above.astype(np.float64)) / 2
            stats["ties"] += int((pos.astype(np.float64) == mid).sum())
    if fmt != "f32":
        assert stats["rounded"] >= 0.05 * stats["values"], stats      # real 16-bit rounding
        assert stats["ties"] >= 20, stats
    # heads: logits and the value conv channel exact, the fmaf chain of the value exact
    assert (np.abs(h) @ np.abs(head_p.astype(np.float64))).max() < (EXACT / 8 if sym else EXACT)
    vcell = h @ head_v.astype(np.float64)
    assert (np.abs(h) @ np.abs(head_v.astype(np.float64))).max() < EXACT
    q = min(2.0 ** np.floor(np.log2(np.abs(x))) for x in list(fc_w[fc_w != 0]) + [fc_b] if x != 0)
    assert (q * 2 ** 40 == np.round(q * 2 ** 40)) and (fc_w / q == np.round(fc_w / q)).all() and fc_b / q == np.round(fc_b / q)
    arg = np.abs(vcell.reshape(len(h), 49) * fc_w).sum(axis=1) + abs(fc_b)
    assert (arg / q).max() < EXACT and arg.max() < 4.0, arg.max()
    # asymmetric weights and boards
    w0 = layers[0][0]
    assert not np.array_equal(w0, w0[::-1]) and not np.array_equal(w0, w0[:, ::-1]) and not np.array_equal(w0, w0.transpose(1, 0, 2, 3))
    fw = fc_w.reshape(7, 7)
    assert not np.array_equal(fw, fw.T) and not np.array_equal(fw, fw[::-1]) and not np.array_equal(fw, fw[:, ::-1])
    feats = np.asarray(features)
    assert any(not np.array_equal(net_oracle.apply_symmetry(f, s), f) for f in feats for s in range(1, 8)) or len(feats) <= 2
    return stats


# ---------------------------------------------------------------- the boards and nets of tests/test_gpu_net_exact.py

ASYM_BLOCKERS = (1 << 0) | (1 << 9) | (1 << 33)     # no dihedral symmetry maps this mask to itself
BLOCK4_MASK = sum(1 << (x + 7 * (6 - y)) for x, y in [(3, 2), (2, 3), (4, 3), (3, 4)])
MASKS = (BLOCK4_MASK, ASYM_BLOCKERS)


def _bits(cells):
    return sum(1 << (x + 7 * (6 - y)) for x, y in cells)


def edge_boards(seed=0, n=29):
    """n (prime: a partial workgroup of 3 and of 6) (mover, opponent) boards: empty, full, pieces only on the edge rows
    and columns, the corners, single edge lines, then random asymmetric boards"""
    all_cells = [(x, y) for x in range(7) for y in range(7)]
    edge = [(x, y) for x, y in all_cells if x in (0, 6) or y in (0, 6)]
    corners = [(0, 0), (0, 6), (6, 0), (6, 6)]
    fixed = [
        (0, 0),
        (_bits(all_cells[::2]), _bits(all_cells[1::2])),
        (_bits(edge[::2]), _bits(edge[1::2])),
        (_bits(corners[:3]), _bits(corners[3:])),
        (_bits([(x, 0) for x in range(7)]), _bits([(6, y) for y in range(1, 7)])),
        (_bits([(0, y) for y in range(7)]), _bits([(x, 6) for x in range(1, 6)])),
        (_bits(edge), 0),
    ]
    rng = np.random.default_rng(seed)
    out = list(fixed)
    while len(out) < n:
        cells = rng.permutation(49)
        k1, k2 = rng.integers(1, 22, size=2)
        out.append((sum(1 << int(c) for c in cells[:k1]), sum(1 << int(c) for c in cells[k1:k1 + k2])))
    return np.array(out[:n], dtype=np.uint64)


def features(lb, masks=MASKS):
    """the boards under every blocker mask, stacked in that order"""
    return np.concatenate([net_oracle.features_from_leaf_boards(lb, m) for m in masks])


def sym_features(lb, masks=MASKS):
    return np.stack([net_oracle.apply_symmetry(f, s) for f in features(lb, masks) for s in range(8)])


# (blocks, filters, fmt, seed): the nets tests/test_gpu_net_exact.py runs on edge_boards() under both masks; the
# block counts 0, 1, 2, 12 and a deep bf16 net (the ring of weight fragments runs past the last layer into padding)
TOWER_CASES = ([(b, 128, fmt, 100 + b) for b in (0, 1, 2, 12) for fmt in ("bf16", "f16", "f32")] + [(40, 128, "bf16", 140)] +
               [(b, f, fmt, 200 + f + b) for f, b in ((64, 3), (256, 2)) for fmt in ("bf16", "f16", "f32")])
SYM_CASES = [(2, 128, fmt, 300) for fmt in ("bf16", "f16", "f32")]
SYM_BOARDS = 5


@functools.lru_cache(maxsize=None)
def tower_net(blocks, filters, fmt, seed):
    """the net of a TOWER_CASES entry, preconditions checked on its boards -> (conv, bn, leaf boards)"""
    lb = edge_boards()
    feats = features(lb)
    conv, bn = make_net(blocks, filters, feats, fmt, seed)
    check_preconditions(conv, bn, feats, fmt)
    return conv, bn, lb


@functools.lru_cache(maxsize=None)
def sym_net(blocks, filters, fmt, seed):
    """the net of a SYM_CASES entry, calibrated and checked on the eight images of its boards"""
    lb = edge_boards(seed=1)[2:2 + SYM_BOARDS]
    feats = sym_features(lb)
    conv, bn = make_net(blocks, filters, feats, fmt, seed, big_head=False)
    check_preconditions(conv, bn, feats, fmt, sym=True)
    return conv, bn, lb
