"""ORACLE — TEST INFRASTRUCTURE ONLY.

CPU restatement of the reference network's forward pass (model.py:38-79,116-142)
in numpy.  PARITY UNPINNED at this boundary: the reference arithmetic lives in
TensorFlow 1.x (tf.nn.conv2d, tf.layers.batch_normalization, tf.matmul, tf.nn.tanh;
unpinned version, absent from this image and from /root/reference), and the
reference holds no golden vector or saved model for it.  This file
restates the published semantics of those ops:

  conv2d NHWC/HWIO, stride 1, padding SAME, cross-correlation:
      out[n,x,y,o] = sum_{i,j,c} in[n, x+i-1, y+j-1, c] * W[i,j,c,o]   (zero outside)
  batch_normalization inference: (x - moving_mean) / sqrt(moving_variance + 1e-3),
      gamma = 1, beta = 0 (not saved by model.save_model: SURVEY.md appendix B, Q1)
  value = tanh(reshape(conv1x1(h), [N,49]) @ fc_w + fc_b)

float64 by default (the 1e-5 gate of the HIP f32 path is checked against this).  Imported by tests/ and
__graft_entry__.smoke() only: bench.py's cpu_baseline is tools/cpu_baseline, not this file.
"""
import numpy as np

BN_EPS = 1e-3


def features_from_leaf_boards(leaf_boards, blockers, dtype=np.float64):
    """(n,2) u64 (mover, opponent) -> (n,7,7,4), cpp/self_play_client.cpp:174-202."""
    leaf_boards = np.asarray(leaf_boards, dtype=np.uint64).reshape(-1, 2)
    n = len(leaf_boards)
    out = np.zeros((n, 7, 7, 4), dtype=dtype)
    out[..., 0] = 1
    for x in range(7):
        for y in range(7):
            sq = x + 7 * (6 - y)
            out[:, x, y, 1] = (leaf_boards[:, 0] >> np.uint64(sq)) & np.uint64(1)
            out[:, x, y, 2] = (leaf_boards[:, 1] >> np.uint64(sq)) & np.uint64(1)
            out[:, x, y, 3] = (int(blockers) >> sq) & 1
    return out


def conv2d_same(x, w):
    """x (n,7,7,c), w (k,k,c,o) -> (n,7,7,o); model.py:118 / :68 / :74."""
    if w.shape[0] == 1:
        return x @ w[0, 0]
    n, c = x.shape[0], x.shape[3]
    xp = np.zeros((n, 9, 9, c), dtype=x.dtype)
    xp[:, 1:8, 1:8, :] = x
    # im2col with k index (i, j, c), matching w.reshape(9c, o)
    cols = np.concatenate([xp[:, i:i + 7, j:j + 7, :] for i in range(3) for j in range(3)], axis=3)
    return (cols.reshape(n * 49, 9 * c) @ w.reshape(9 * c, w.shape[3])).reshape(n, 7, 7, -1)


def batch_norm(x, mean, var):
    return (x - mean) / np.sqrt(var + BN_EPS)


def forward(conv_weights, bn_params, features, dtype=np.float64):
    """-> (policy logits (n,7,7,17), value (n,1)); model.py:38-79."""
    cw = [np.asarray(a, dtype=dtype) for a in conv_weights]
    bn = [np.asarray(a, dtype=dtype) for a in bn_params]
    blocks = (len(cw) - 5) // 2
    h = np.asarray(features, dtype=dtype)
    h = np.maximum(batch_norm(conv2d_same(h, cw[0]), bn[0], bn[1]), 0)          # model.py:56-57
    for b in range(blocks):                                                      # model.py:132-142
        i1, i2 = 1 + 2 * b, 2 + 2 * b
        t = np.maximum(batch_norm(conv2d_same(h, cw[i1]), bn[2 * i1], bn[2 * i1 + 1]), 0)
        t = batch_norm(conv2d_same(t, cw[i2]), bn[2 * i2], bn[2 * i2 + 1])
        h = np.maximum(t + h, 0)
    policy = conv2d_same(h, cw[2 * blocks + 1])                                  # model.py:66-69
    v = conv2d_same(h, cw[2 * blocks + 2]).reshape(len(h), 49)                   # model.py:71-75
    value = np.tanh(v @ cw[2 * blocks + 3] + cw[2 * blocks + 4])                 # model.py:76-79
    return policy, value


def apply_symmetry(tensor, symmetry):
    """The dihedral image `symmetry` (0..7) of a (7,7,k) tensor as nn_evals.py:8-16 defines it: bit 0 mirrors the first
    axis, bit 1 the second, bit 2 then swaps the two."""
    axes = [axis for axis, bit in ((0, 1), (1, 2)) if symmetry & bit]
    image = np.flip(tensor, axis=axes) if axes else tensor
    return np.swapaxes(image, 0, 1) if symmetry & 4 else image


# inverse of every image under composition (nn_evals.py:27): the two mirror-then-swap images 5 and 6 undo each other
INVERSE_SYMMETRY = {s: (s if s not in (5, 6) else 11 - s) for s in range(8)}


def sym_average(evaluate, features):
    """nn_evals.evaluate (nn_evals.py:48-62) for a batch, around any evaluator `evaluate(images (m,7,7,4)) ->
    (policy (m,7,7,17), value (m,1))`: the evaluator on the 8 dihedral images of every board, policies brought back
    with the inverse symmetry (spatial axes only) and averaged, values averaged.  Pinned by
    tests/golden/nn_evals_sym.npz (the reference's own nn_evals.evaluate around the same injected evaluator)."""
    n = len(features)
    images = np.stack([apply_symmetry(f, s) for f in features for s in range(8)])
    policy, value = evaluate(images)
    policy = np.asarray(policy).reshape(n, 8, 7, 7, 17)
    back = np.stack([np.stack([apply_symmetry(policy[i, s], INVERSE_SYMMETRY[s]) for s in range(8)]) for i in range(n)])
    return back.mean(axis=1), np.asarray(value).reshape(n, 8).mean(axis=1).reshape(n, 1)


def forward_sym(conv_weights, bn_params, features, dtype=np.float64):
    """sym_average around the restated net.  -> (policy (n,7,7,17), value (n,1))."""
    features = np.asarray(features, dtype=dtype)
    return sym_average(lambda images: forward(conv_weights, bn_params, images, dtype=dtype), features)


# ---------------------------------------------------------------- the 16-bit towers' arithmetic, rounding for rounding
#
# forward_lowp restates what the HIP towers (ataxxzero_amd/csrc/net_kernels.hip) compute, in float64 with a rounding at
# exactly the places where the kernels round (line numbers of net_kernels.hip):
#   batch norm   azh_net_create :1683-1685: inv = 1/sqrt(double(var) + double(eps)), eps arriving as a float (link.Net
#                passes a c_float); scale = float(inv), shift = float(-double(mean) * inv)
#   conv weights pack_conv :1444, pack_conv16 :1464, the im2col first layer :1567 (net_pack): the float product
#                w * scale, rounded once to bf16 / f16 (f32_to_bf16 :1419, f32_to_f16 :1429: round to nearest even)
#   head weights net_pack :1528: the policy and value 1x1 convolutions rounded to 16 bits without a scale
#   input planes exact 0 / 1
#   each layer   the f32 accumulator starts at the shift (:248, :860) plus, for a block's second convolution, the
#                stored 16-bit residual input (:274, :887), and sums the products; the epilogue converts the sum to 16
#                bits with round to nearest even (__builtin_convertvector, :442, relu_pack :763) and applies ReLU.
#                ReLU is IEEE's maximum with 0, here and in the kernels: a NaN stays a NaN, +inf stays +inf, -inf and -0
#                give a zero.  For numbers it commutes with the conversion; for a NaN it does not commute with every
#                way of taking it: the bf16 16x16x32 towers (k_tower2, k_tower2_thin, k_tower2_pair) take a packed
#                integer max on the converted pair and clear the NaN the device generates, whose sign bit is set
#                (relu_pack :760).  That behaviour is the defect "relu_erases_negative_nan_only" below, and
#                tests/test_gpu_net_edges.py pins the bf16 towers to it bit for bit.
#   edges        measured on the MI355X (tests/test_gpu_net_edges.py on the nets of tests/net_edges.py): the MFMAs keep
#                subnormal 16-bit and f32 operands and accumulators, the conversions round ties to even down to half the
#                smallest subnormal and overflow to infinity at the tie (65520 in f16), tanhf returns a subnormal argument
#                and +-1 for an infinite one — all as numpy computes them below, so no hardware switch exists here.  The
#                NaN the device generates is 0xFFC00000; a NaN is compared as a NaN, whatever its sign.
#   outputs      logits = the f32 head accumulators (:595; tower2_run); the value conv channel stays f32 (:597);
#                value = tanhf(s + fc_b), s the fmaf chain over c = 7 x + y of vcell[c] * fc_w[c] (:607-608, :1347-1348)
# The sums themselves are taken in float64 and rounded to float once: on nets whose products and partial sums are all
# exact in f32 (tests/net_exact.py) that IS the kernels' accumulator in every summation order; elsewhere the two differ
# by accumulation-order noise.  fmt "f32" is the f32 tower (the same folding, no 16-bit rounding anywhere).

LOWP_FORMATS = ("f32", "bf16", "f16")
# The sign bit of the NaN that the MI355X generates (inf - inf, 0 * inf; matrix unit and adders, every format): the pattern
# is 0xFFC00000, measured by tests/test_gpu_net_edges.py on the overflow nets.  Only a ReLU taken on bit patterns can tell.
GENERATED_NAN_SIGN_BIT = 1


def round_bf16(x):
    """float32 array -> the nearest bf16 values (round to nearest even), as float32.  Bit for bit the host's f32_to_bf16:
    NaN stays a (quiet) NaN, overflow goes to infinity."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    r = np.where(nan, u | np.uint32(0x00400000), r) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def round_f16(x):
    """float32 array -> the nearest IEEE half values (round to nearest even, subnormals kept, overflow to infinity), as
    float32; integer operations on the float32 encoding."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    sign = (u >> 16) & 0x8000
    a = u & 0x7FFFFFFF
    # normal halves (|x| >= 2^-14): keep 10 of the 23 fraction bits, ties to the even neighbour, rebias 127 -> 15
    h_norm = ((a + 0xFFF + ((a >> 13) & 1)) >> 13) - (112 << 10)
    # subnormal halves: |x| / 2^-24 rounded to an integer, ties to even
    e = a >> 23
    m = (a & 0x7FFFFF) | 0x800000
    s = np.clip(126 - e, 1, 31)
    q = m >> s
    rem = m & ((1 << s) - 1)
    half = 1 << (s - 1)
    h_sub = q + ((rem > half) | ((rem == half) & (q & 1 == 1)))
    h = np.where(a >= 0x38800000, h_norm, np.where(e >= 102, h_sub, 0))
    h = np.where(a >= 0x477FF000, 0x7C00, h)            # >= 65520: infinity
    h = np.where(a > 0x7F800000, 0x7E00, h)             # NaN
    return ((sign | h).astype(np.uint16)).view(np.float16).astype(np.float32)


def _rounder(fmt):
    if fmt not in LOWP_FORMATS:
        raise ValueError("fmt must be one of %s, got %r" % (LOWP_FORMATS, fmt))
    return {"f32": lambda x: np.asarray(x, dtype=np.float32), "bf16": round_bf16, "f16": round_f16}[fmt]


def bn_constants(mean, var, eps=BN_EPS):
    """(scale, shift) as float32, as azh_net_create derives them (net_kernels.hip:1683-1685)."""
    inv = 1.0 / np.sqrt(np.asarray(var, np.float32).astype(np.float64) + np.float64(np.float32(eps)))
    return inv.astype(np.float32), (-np.asarray(mean, np.float32).astype(np.float64) * inv).astype(np.float32)


def lowp_parameters(conv_weights, bn_params, fmt, eps=BN_EPS):
    """The net as the towers hold it: [(16-bit folded weights (3,3,c,o), f32 shift (o,))] per tower layer, the 16-bit
    policy (c,17) and value (c,) head weights, fc_w (49,) and fc_b as float32 — every entry a float32 value."""
    rnd = _rounder(fmt)
    cw = [np.asarray(a, dtype=np.float32) for a in conv_weights]
    blocks = (len(cw) - 5) // 2
    layers = []
    for i in range(2 * blocks + 1):
        scale, shift = bn_constants(bn_params[2 * i], bn_params[2 * i + 1], eps)
        layers.append((rnd(cw[i] * scale), shift))                       # f32 product, one rounding (pack_conv)
    head_p = rnd(cw[2 * blocks + 1][0, 0])                                # net_pack: heads unscaled
    head_v = rnd(cw[2 * blocks + 2][0, 0, :, 0])
    return layers, head_p, head_v, cw[2 * blocks + 3].reshape(49), np.float32(cw[2 * blocks + 4].reshape(-1)[0])


def _truncate_bf16(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _truncate_f16(x):
    x = np.asarray(x, dtype=np.float32)
    t = round_f16(x).astype(np.float16)
    return np.where(np.abs(t.astype(np.float32)) > np.abs(x), np.nextafter(t, np.float16(0)), t).astype(np.float32)


# smallest normal, smallest subnormal and largest finite value of each tower format (activations and folded weights)
FORMAT_LIMITS = {"f32": (2.0 ** -126, 2.0 ** -149, float(np.finfo(np.float32).max)),
                 "bf16": (2.0 ** -126, 2.0 ** -133, (2.0 - 2.0 ** -7) * 2.0 ** 127),
                 "f16": (2.0 ** -14, 2.0 ** -24, 65504.0)}


def _flush_subnormals(x, fmt):
    """values below the format's smallest normal become zeros of their sign"""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.abs(x) < FORMAT_LIMITS[fmt][0], np.copysign(0.0, x), x)


def _only_tap(w, i, j):
    out = np.zeros_like(w)
    out[i, j] = w[i, j]
    return out


def _forward_lowp(conv_weights, bn_params, features, fmt, eps=BN_EPS, defect=None, with_argument=False):
    """forward_lowp with an optional deliberate `defect` (the mutants of tests/test_net_emulation.py and
    tests/test_net_edges_host.py: what a subtly wrong kernel would compute).
    -> (policy (n,7,7,17), value (n,1), activations per tower layer[, the f32 argument of tanh (n,1) with_argument])."""
    with np.errstate(invalid="ignore", over="ignore"):       # infinities and NaNs are ordinary values here
        return _forward_lowp_body(conv_weights, bn_params, features, fmt, eps, defect, with_argument)


def _forward_lowp_body(conv_weights, bn_params, features, fmt, eps, defect, with_argument):
    rnd = _rounder(fmt)
    f32 = np.float32
    layers, head_p, head_v, fc_w, fc_b = lowp_parameters(conv_weights, bn_params, fmt, eps)
    if defect == "scale_after_rounding":
        cw = [np.asarray(a, dtype=np.float32) for a in conv_weights]
        layers = [(rnd(rnd(cw[i]) * bn_constants(bn_params[2 * i], bn_params[2 * i + 1], eps)[0]), sh)
                  for i, (_, sh) in enumerate(layers)]
    if defect == "truncate" and fmt != "f32":
        rnd = _truncate_bf16 if fmt == "bf16" else _truncate_f16
    if defect == "flush_subnormal_inputs":
        # a matrix unit that reads subnormal A / B operands as zeros: weights here, activations where a layer reads them
        layers = [(_flush_subnormals(w, fmt), sh) for w, sh in layers]
        head_p, head_v = _flush_subnormals(head_p, fmt), _flush_subnormals(head_v, fmt)
    h = np.asarray(features, dtype=np.float64)
    acts = []

    def relu(out):
        """IEEE, what the kernels' epilogues are held to: a NaN stays a NaN, +inf stays +inf, -inf and -0 give a zero"""
        if defect == "relu_erases_nan":
            return np.where(out > 0, out, 0.0)               # "v > 0 ? v : 0": every NaN becomes 0
        if defect == "relu_erases_negative_nan_only":
            # a packed integer max with 0 on the 16-bit pattern: clears what has the sign bit set, a NaN included, and
            # keeps a NaN whose sign bit is clear.  No NaN enters these towers from outside (non-finite tower weights are
            # refused), so every NaN is one the arithmetic generated, and its sign is GENERATED_NAN_SIGN_BIT — the
            # device's, not this host's.  With the bit set this mutant is what the bf16 16x16x32 towers compute today,
            # and it coincides with relu_erases_nan; with the bit clear it would be the faithful ReLU.
            erased = np.isnan(out) if GENERATED_NAN_SIGN_BIT else np.zeros(out.shape, dtype=bool)
            return np.where(erased, 0.0, np.maximum(out, 0))
        return np.maximum(out, 0)

    def to_format(z):
        """the f32 accumulator, converted to the format"""
        z32 = np.asarray(z, dtype=np.float64).astype(np.float32)
        out = rnd(z32).astype(np.float64)
        if defect == "saturate_overflow":
            over = np.isinf(out) & np.isfinite(z)
            out = np.where(over, np.copysign(FORMAT_LIMITS[fmt][2], z), out)
        if defect == "flush_subnormal_outputs":
            out = _flush_subnormals(out, fmt)
        return out

    def layer(x, w, shift, residual=None, index=0):
        if defect == "flush_subnormal_inputs":
            x = _flush_subnormals(x, fmt)
        z = conv2d_same(x, w.astype(np.float64))
        if defect == "edge_tap" and index > 0:
            # one on-board tap (dx = +1, dy = 0) missing for the cells of the y = 0 edge
            zt = conv2d_same(x, _only_tap(w.astype(np.float64), 2, 1))
            z[:, :, 0, :] -= zt[:, :, 0, :]
        z = z + shift.astype(np.float64)
        if residual is not None and defect != "residual_after_rounding":
            z = z + residual
        out = to_format(z)
        if residual is not None and defect == "residual_after_rounding":
            out = to_format(out + residual)
        return relu(out)

    blocks = (len(layers) - 1) // 2
    h = layer(h, *layers[0])
    acts.append(h)
    for b in range(blocks):
        t = layer(h, *layers[1 + 2 * b], index=1 + 2 * b)
        acts.append(t)
        h = layer(t, *layers[2 + 2 * b], residual=h, index=2 + 2 * b)
        acts.append(h)
    hh = _flush_subnormals(h, fmt) if defect == "flush_subnormal_inputs" else h
    policy = (hh @ head_p.astype(np.float64)).astype(np.float32)
    vcell = (hh @ head_v.astype(np.float64)).astype(np.float32)            # (n,7,7), f32
    if defect == "policy16_from_value_row":
        policy[..., 16] = vcell
    v = (np.swapaxes(vcell, 1, 2) if defect == "value_xy_swapped" else vcell).reshape(len(h), 49)
    s = np.zeros(len(h), dtype=np.float32)
    for c in range(49):                                                   # fmaf chain, c = 7 x + y (model.py:75)
        s = (v[:, c].astype(np.float64) * np.float64(fc_w[c]) + s.astype(np.float64)).astype(f32)
    arg = (s + fc_b).astype(f32).astype(np.float64).reshape(-1, 1)
    value = np.tanh(arg)                                     # tanh(+-inf) = +-1, tanh(NaN) a NaN, tanh(-0) = -0
    out = (policy.astype(np.float64) + 0.0, value, acts)     # (+ 0.0: a zero logit is +0, as the kernels write it)
    return out + (arg,) if with_argument else out


def forward_lowp(conv_weights, bn_params, features, fmt, eps=BN_EPS):
    """The tower of dtype `fmt` ("f32", "bf16", "f16") restated rounding for rounding (see above).
    -> (policy logits (n,7,7,17), value (n,1)) in float64; the logits are float32 values, the value is the float64
    tanh of the kernels' float32 argument (their tanhf is within a few ulp of it)."""
    policy, value, _ = _forward_lowp(conv_weights, bn_params, features, fmt, eps)
    return policy, value


def forward_lowp_sym(conv_weights, bn_params, features, fmt, eps=BN_EPS):
    """sym_average around forward_lowp: the symmetry-averaged towers (azh_net_launch with symmetry scratch + k_sym_reduce, whose f32 sum
    of eight logits times 0.125 is exact wherever the eight logits are exact integers of magnitude < 2^21)."""
    features = np.asarray(features, dtype=np.float64)
    return sym_average(lambda images: forward_lowp(conv_weights, bn_params, images, fmt, eps), features)
