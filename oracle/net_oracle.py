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
#   batch norm   azh_net_create :1643-1646: inv = 1/sqrt(double(var) + double(eps)), eps arriving as a float (link.Net
#                passes a c_float); scale = float(inv), shift = float(-double(mean) * inv)
#   conv weights pack_conv :1423-1440, pack_conv16 :1443-1458, the im2col first layer :1528-1537: the float product
#                w * scale, rounded once to bf16 / f16 (f32_to_bf16 :1398, f32_to_f16 :1408: round to nearest even)
#   head weights net_pack :1490-1495: the policy and value 1x1 convolutions rounded to 16 bits without a scale
#   input planes exact 0 / 1
#   each layer   the f32 accumulator starts at the shift (:246, :832-842) plus, for a block's second convolution, the
#                stored 16-bit residual input (:272, :868), and sums the products; the epilogue converts the sum to 16
#                bits with round to nearest even (__builtin_convertvector, :439, :766) and applies ReLU, which commutes
#                with the conversion (:746-750)
#   outputs      logits = the f32 head accumulators (:591, :1313-1315); the value conv channel stays f32 (:593, :1316);
#                value = tanhf(s + fc_b), s the fmaf chain over c = 7 x + y of vcell[c] * fc_w[c] (:603-604, :1326-1327)
# The sums themselves are taken in float64 and rounded to float once: on nets whose products and partial sums are all
# exact in f32 (tests/net_exact.py) that IS the kernels' accumulator in every summation order; elsewhere the two differ
# by accumulation-order noise.  fmt "f32" is the f32 tower (the same folding, no 16-bit rounding anywhere).

LOWP_FORMATS = ("f32", "bf16", "f16")


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
    """(scale, shift) as float32, as azh_net_create derives them (net_kernels.hip:1634-1650)."""
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


def _only_tap(w, i, j):
    out = np.zeros_like(w)
    out[i, j] = w[i, j]
    return out


def _forward_lowp(conv_weights, bn_params, features, fmt, eps=BN_EPS, defect=None):
    """forward_lowp with an optional deliberate `defect` (tests/test_net_emulation.py's mutants: what a subtly wrong
    kernel would compute).  -> (policy (n,7,7,17), value (n,1), activations per tower layer)."""
    rnd = _rounder(fmt)
    f32 = np.float32
    layers, head_p, head_v, fc_w, fc_b = lowp_parameters(conv_weights, bn_params, fmt, eps)
    if defect == "scale_after_rounding":
        cw = [np.asarray(a, dtype=np.float32) for a in conv_weights]
        layers = [(rnd(rnd(cw[i]) * bn_constants(bn_params[2 * i], bn_params[2 * i + 1], eps)[0]), sh)
                  for i, (_, sh) in enumerate(layers)]
    if defect == "truncate" and fmt != "f32":
        rnd = _truncate_bf16 if fmt == "bf16" else _truncate_f16
    h = np.asarray(features, dtype=np.float64)
    acts = []

    def layer(x, w, shift, residual=None, index=0):
        z = conv2d_same(x, w.astype(np.float64))
        if defect == "edge_tap" and index > 0:
            # one on-board tap (dx = +1, dy = 0) missing for the cells of the y = 0 edge
            zt = conv2d_same(x, _only_tap(w.astype(np.float64), 2, 1))
            z[:, :, 0, :] -= zt[:, :, 0, :]
        z = z + shift.astype(np.float64)
        if residual is not None and defect != "residual_after_rounding":
            z = z + residual
        out = rnd(z.astype(np.float32)).astype(np.float64)
        if residual is not None and defect == "residual_after_rounding":
            out = rnd((out + residual).astype(np.float32)).astype(np.float64)
        return np.maximum(out, 0)

    blocks = (len(layers) - 1) // 2
    h = layer(h, *layers[0])
    acts.append(h)
    for b in range(blocks):
        t = layer(h, *layers[1 + 2 * b], index=1 + 2 * b)
        acts.append(t)
        h = layer(t, *layers[2 + 2 * b], residual=h, index=2 + 2 * b)
        acts.append(h)
    policy = (h @ head_p.astype(np.float64)).astype(np.float32)
    vcell = (h @ head_v.astype(np.float64)).astype(np.float32)             # (n,7,7), f32
    if defect == "policy16_from_value_row":
        policy[..., 16] = vcell
    v = (np.swapaxes(vcell, 1, 2) if defect == "value_xy_swapped" else vcell).reshape(len(h), 49)
    s = np.zeros(len(h), dtype=np.float32)
    for c in range(49):                                                   # fmaf chain, c = 7 x + y (model.py:75)
        s = (v[:, c].astype(np.float64) * np.float64(fc_w[c]) + s.astype(np.float64)).astype(f32)
    value = np.tanh((s + fc_b).astype(f32).astype(np.float64)).reshape(-1, 1)
    return policy.astype(np.float64) + 0.0, value, acts      # (+ 0.0: a zero logit is +0, as the kernels write it)


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
