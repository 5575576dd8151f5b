"""REFERENCE — TEST INFRASTRUCTURE ONLY.

One optimisation step of training.train() restated in plain numpy, float64 by default, with a hand-derived backward: the
training-mode forward of model.py:38-79 on batch statistics, the two heads of Network._heads and the three of
Network._aux_heads, the losses of training.losses and training._aux_loss_terms as their docstrings state them, the analytic
gradient of their weighted sum, the momentum update and the moving batch-norm statistics.  Features are NHWC and weights
HWIO as in oracle/net_oracle.py, whose conv2d_same is the convolution here; the auxiliary arrays come and go in the layout of
Network.aux_to_numpy (the sidecar's).

    forward    per BN layer mu, var = mean and BIASED variance of the convolution's output over (n, x, y);
               y = gamma * (z - mu) / sqrt(var + 1e-3) + beta  (gamma = 1, beta = 0 unless `affine` is given)
    losses     policy: -sum_k p_k log softmax(logits)_k over the 833 cells, mean over samples;  value: mean (z - v)^2;
               reg: 1e-4 * sum_w sum(w^2) / 2 over EVERY trainable tensor (fc bias, auxiliary heads, gamma / beta included);
               ownership: sum_i w_i mean_49 (tanh(a_0) - own)^2 / max(1, sum w),  score: sum_i w_i (s_i - score_i / 49)^2 /
               max(1, sum w) with w = aux_weight[:, 0];  reply: sum_i w_i CE_i / max(1, sum w) with w = aux_weight[:, 1]
    step       g = d(policy + value + reg + a_own * ownership + a_score * score + a_reply * reply) / dw;
               v <- 0.9 v + g,  w <- w - lr v  (v = 0 before the first step)
    statistics moving mean <- 0.99 m + 0.01 mu;  moving variance <- 0.99 s + 0.01 * var * n / (n - 1),  n = batch * 49

The moving variance takes the UNBIASED batch variance although the forward normalises with the biased one: that is torch's
documented rule for BatchNorm2d's running_var, so it is what the trainer writes into the `.npy`; the reference's TensorFlow 1
arithmetic is not available to check against (`unbiased=False` gives the other rule, for tests that must tell the two apart).

The gradient is analytic on purpose.  Central differences of this very loss were off by 3e-2 .. 2e-6 for h = 1e-4 .. 1e-8: a
perturbed convolution weight pushes some of the thousands of pre-activations across a ReLU kink.

`dtype=np.float32` runs the same code in float32: its distance to the float64 run is what tests allow a float32 trainer.
"""
import numpy as np

from oracle.net_oracle import conv2d_same

BN_EPS = 1e-3
BN_MOMENTUM = 0.01
MOMENTUM = 0.9
L2 = 1e-4
CELLS = 49
AUX_KEYS = ("aux_conv", "aux_fc_weight", "aux_fc_bias", "reply_conv")


# ---------------------------------------------------------------- pieces: forward and backward of each operation

def _im2col(x):
    """(n,7,7,c) -> (n*49, 9c), k index (i, j, c) as conv2d_same's."""
    n, c = x.shape[0], x.shape[3]
    xp = np.zeros((n, 9, 9, c), dtype=x.dtype)
    xp[:, 1:8, 1:8, :] = x
    return np.concatenate([xp[:, i:i + 7, j:j + 7, :] for i in range(3) for j in range(3)], axis=3).reshape(n * CELLS, 9 * c)


def _conv_backward(x, w, dz, need_dx=True):
    """-> (dw, dx) of z = conv2d_same(x, w) given dz."""
    n, c, o = x.shape[0], x.shape[3], w.shape[3]
    if w.shape[0] == 1:
        dw = (x.reshape(n * CELLS, c).T @ dz.reshape(n * CELLS, o)).reshape(w.shape)
        return dw, (dz @ w[0, 0].T if need_dx else None)
    dz2 = dz.reshape(n * CELLS, o)
    dw = (_im2col(x).T @ dz2).reshape(w.shape)
    if not need_dx:
        return dw, None
    dcols = (dz2 @ w.reshape(9 * c, o).T).reshape(n, 7, 7, 9, c)
    dxp = np.zeros((n, 9, 9, c), dtype=x.dtype)
    for k in range(9):
        i, j = divmod(k, 3)
        dxp[:, i:i + 7, j:j + 7, :] += dcols[:, :, :, k, :]
    return dw, dxp[:, 1:8, 1:8, :]


def _bn_forward(z, gamma_beta, f):
    mu = z.mean(axis=(0, 1, 2))
    var = z.var(axis=(0, 1, 2))                                            # biased: divided by n
    inv = f(1.0) / np.sqrt(var + f(BN_EPS))
    xhat = (z - mu) * inv
    y = xhat if gamma_beta is None else xhat * gamma_beta[0] + gamma_beta[1]
    return y, (xhat, inv), mu, var


def _bn_backward(dy, kept, gamma_beta, f):
    """-> (dz, (dgamma, dbeta)) through the batch statistics."""
    xhat, inv = kept
    count = f(xhat.shape[0] * CELLS)
    dgamma, dbeta = (dy * xhat).sum(axis=(0, 1, 2)), dy.sum(axis=(0, 1, 2))
    dxhat = dy if gamma_beta is None else dy * gamma_beta[0]
    s1, s2 = dxhat.sum(axis=(0, 1, 2)), (dxhat * xhat).sum(axis=(0, 1, 2))
    return inv / count * (count * dxhat - s1 - xhat * s2), (dgamma, dbeta)


def _cross_entropy(logits, target):
    """Per sample -sum_k target_k log softmax(logits)_k over the flattened cells -> (per sample, d per sample / d logits)."""
    n = logits.shape[0]
    z, t = logits.reshape(n, -1), target.reshape(n, -1)
    shifted = z - z.max(axis=1, keepdims=True)
    logp = shifted - np.log(np.exp(shifted).sum(axis=1, keepdims=True))
    return -(t * logp).sum(axis=1), (np.exp(logp) * t.sum(axis=1, keepdims=True) - t).reshape(logits.shape)


# ---------------------------------------------------------------- the parameters

def _as_params(conv, aux, affine, dtype):
    """The trainable tensors in the restatement's layouts: the `.npy` list as it is; the heads' 1x1 convolutions HWIO and
    their Linear (49, 1)."""
    p = {"conv": [np.array(a, dtype=dtype) for a in conv], "aux": None, "affine": None}
    if aux is not None:
        p["aux"] = [np.array(np.transpose(aux["aux_conv"], (2, 3, 1, 0)), dtype=dtype),
                    np.array(np.asarray(aux["aux_fc_weight"]).reshape(CELLS, 1), dtype=dtype),
                    np.array(aux["aux_fc_bias"], dtype=dtype).reshape(1),
                    np.array(np.transpose(aux["reply_conv"], (2, 3, 1, 0)), dtype=dtype)]
    if affine is not None:
        p["affine"] = [[np.array(g, dtype=dtype), np.array(b, dtype=dtype)] for g, b in affine]
    return p


def _leaves(p):
    """Every trainable tensor of a parameter (or gradient) set, in one fixed order."""
    out = list(p["conv"])
    if p["aux"] is not None:
        out += p["aux"]
    if p["affine"] is not None:
        out += [a for pair in p["affine"] for a in pair]
    return out


def _aux_out(arrays):
    a, fw, fb, r = arrays
    return {"aux_conv": np.ascontiguousarray(np.transpose(a, (3, 2, 0, 1))), "aux_fc_weight": fw.reshape(1, CELLS).copy(),
            "aux_fc_bias": fb.copy(), "reply_conv": np.ascontiguousarray(np.transpose(r, (3, 2, 0, 1)))}


# ---------------------------------------------------------------- loss and gradient of one minibatch

def loss_and_gradient(p, batch, aux_loss_weights, dtype=np.float64):
    """-> (loss terms: three, or six with auxiliary heads; gradient of their weighted sum, shaped as p; [(mu, var)] per BN
    layer, var biased; the input of every ReLU)."""
    f = np.dtype(dtype).type
    cw, affine = p["conv"], p["affine"]
    layers = len(cw) - 4
    blocks = (layers - 1) // 2
    w_policy, w_value, fc_w, fc_b = cw[layers:]
    feats, policies, values = (np.asarray(a, dtype=dtype) for a in batch[:3])
    n = feats.shape[0]

    def gb(i):
        return None if affine is None else affine[i]

    # forward, keeping every convolution's input, every BN layer's (xhat, inv) and every ReLU's output
    inputs, kept, stats = [None] * layers, [None] * layers, [None] * layers

    def conv_bn(x, i):
        inputs[i] = x
        y, kept[i], mu, var = _bn_forward(conv2d_same(x, cw[i]), gb(i), f)
        stats[i] = (mu, var)
        return y

    pre = [conv_bn(feats, 0)]                                              # what every ReLU reads
    h = np.maximum(pre[0], 0)
    outs = [h]                                                             # the tower's output after the stem and each block
    mids = []
    for b in range(blocks):
        pre.append(conv_bn(h, 1 + 2 * b))
        t = np.maximum(pre[-1], 0)
        pre.append(conv_bn(t, 2 + 2 * b) + h)
        h = np.maximum(pre[-1], 0)
        mids.append(t)
        outs.append(h)

    grad = {"conv": [None] * len(cw), "aux": None, "affine": None if affine is None else [None] * layers}
    logits = conv2d_same(h, w_policy)
    per_policy, d_logits = _cross_entropy(logits, policies)
    policy_loss = per_policy.mean()
    d_logits = d_logits / f(n)
    v_cells = conv2d_same(h, w_value).reshape(n, CELLS)
    v = np.tanh(v_cells @ fc_w + fc_b)
    value_loss = ((values - v) ** 2).mean()
    d_s = f(2.0) * (v - values) / f(values.size) * (f(1.0) - v * v)
    grad["conv"][layers + 2] = v_cells.T @ d_s
    grad["conv"][layers + 3] = d_s.sum(axis=0)
    grad["conv"][layers], dh = _conv_backward(h, w_policy, d_logits)
    grad["conv"][layers + 1], dh_v = _conv_backward(h, w_value, (d_s @ fc_w.T).reshape(n, 7, 7, 1))
    dh = dh + dh_v
    terms = [policy_loss, value_loss]

    if p["aux"] is not None:
        a_own, a_score, a_reply = (f(w) for w in aux_loss_weights)
        w_aux, afc_w, afc_b, w_reply = p["aux"]
        ownership, score, reply, aux_weight = (np.asarray(a, dtype=dtype) for a in batch[3:7])
        wf, wr = aux_weight[:, 0], aux_weight[:, 1]
        d_final, d_reply = max(f(1.0), wf.sum()), max(f(1.0), wr.sum())
        a = conv2d_same(h, w_aux)
        own = np.tanh(a[..., 0])
        sc_cells = a[..., 1].reshape(n, CELLS)
        sc = sc_cells @ afc_w + afc_b
        per_reply, d_rlogits = _cross_entropy(conv2d_same(h, w_reply), reply)
        own_loss = (wf * ((own - ownership) ** 2).reshape(n, -1).mean(axis=1)).sum() / d_final
        score_loss = (wf * ((sc - score / f(CELLS)) ** 2).reshape(n)).sum() / d_final
        reply_loss = (wr * per_reply).sum() / d_reply
        d_own = a_own * (wf / d_final)[:, None, None] * f(2.0) * (own - ownership) / f(CELLS) * (f(1.0) - own * own)
        d_sc = a_score * (wf / d_final)[:, None] * f(2.0) * (sc - score / f(CELLS))
        d_a = np.stack([d_own, (d_sc @ afc_w.T).reshape(n, 7, 7)], axis=3)
        d_rlogits = d_rlogits * (a_reply * wr / d_reply)[:, None, None, None]
        g_aux, dh_a = _conv_backward(h, w_aux, d_a)
        g_reply, dh_r = _conv_backward(h, w_reply, d_rlogits)
        grad["aux"] = [g_aux, sc_cells.T @ d_sc, d_sc.sum(axis=0), g_reply]
        dh = dh + dh_a + dh_r
        aux_terms = [own_loss, score_loss, reply_loss]

    # backward through the tower
    def conv_bn_backward(dy, i, need_dx=True):
        dz, g_affine = _bn_backward(dy, kept[i], gb(i), f)
        if affine is not None:
            grad["affine"][i] = list(g_affine)
        grad["conv"][i], dx = _conv_backward(inputs[i], cw[i], dz, need_dx)
        return dx

    for b in reversed(range(blocks)):
        d_sum = dh * (outs[b + 1] > 0)                                     # through the ReLU after the residual add
        dt = conv_bn_backward(d_sum, 2 + 2 * b) * (mids[b] > 0)
        dh = conv_bn_backward(dt, 1 + 2 * b) + d_sum
    conv_bn_backward(dh * (outs[0] > 0), 0, need_dx=False)

    reg = f(0.0)
    for w, g in zip(_leaves(p), _leaves(grad)):
        reg = reg + (w * w).sum() / f(2.0)
        g += f(L2) * w.reshape(g.shape)
    terms.append(f(L2) * reg)
    if p["aux"] is not None:
        terms += aux_terms
    return tuple(float(t) for t in terms), grad, stats, pre


def batch_statistics(conv, batch, dtype=np.float64):
    """The batch mean and biased batch variance of every BN layer on one minibatch, in the order of a `.npy`'s second list: what
    the moving statistics of a net in training hover around."""
    _, _, stats, _ = loss_and_gradient(_as_params(conv, None, None, dtype), batch[:3], None, dtype)
    return [a for pair in stats for a in pair]


# ---------------------------------------------------------------- the entry point

def run(conv, bn, aux, batches, lr, aux_loss_weights=None, dtype=np.float64, affine=None, unbiased=True):
    """len(batches) optimisation steps from the net (conv, bn) of a `.npy`, one minibatch each.

    conv, bn: model.load_model's two lists;  aux: the sidecar's four arrays (Network.aux_to_numpy), or None for a net without
    auxiliary heads;  batches: tuples of three arrays (features (n,7,7,4), policies (n,7,7,17), values (n,1)), or seven with
    (ownership (n,7,7), score (n,1) in stones, reply (n,7,7,17), aux_weight (n,2)) behind them;  aux_loss_weights: the weights
    of (ownership, score, reply) in the loss;  affine: [(gamma, beta)] per BN layer, trained like every weight
    (reference_bn_affine), or None;  unbiased: the moving variance's rule (module docstring).
    -> {"conv", "bn", "aux", "affine": as given, after the steps;  "losses": per step the three or six terms, unweighted;
        "relu_inputs": per step what every ReLU of the tower read (kink_margin)}"""
    f = np.dtype(dtype).type
    p = _as_params(conv, aux, affine, dtype)
    moving = [np.array(a, dtype=dtype) for a in bn]
    velocity = [np.zeros_like(w) for w in _leaves(p)]
    history, relu_inputs = [], []
    for batch in batches:
        terms, grad, stats, pre = loss_and_gradient(p, batch, aux_loss_weights, dtype)
        history.append(terms)
        relu_inputs.append(pre)
        for w, v, g in zip(_leaves(p), velocity, _leaves(grad)):
            v *= f(MOMENTUM)
            v += g.reshape(v.shape)
            w -= f(lr) * v
        count = np.asarray(batch[0]).shape[0] * CELLS
        for i, (mu, var) in enumerate(stats):
            if unbiased:
                var = var * (f(count) / f(count - 1))
            moving[2 * i] = f(1.0 - BN_MOMENTUM) * moving[2 * i] + f(BN_MOMENTUM) * mu
            moving[2 * i + 1] = f(1.0 - BN_MOMENTUM) * moving[2 * i + 1] + f(BN_MOMENTUM) * var
    return {"conv": p["conv"], "bn": moving, "aux": None if p["aux"] is None else _aux_out(p["aux"]), "affine": p["affine"],
            "losses": history, "relu_inputs": relu_inputs}


# ---------------------------------------------------------------- minibatches made by hand, and distances between results

def synthetic_batch(rng, n, aux=False, reply_weights=True):
    """A minibatch of the shapes and ranges the trainer meets: boards of ones / mover / opponent / wall planes, Dirichlet
    policies over a few dozen cells, values +-1 and blended fractions, ownership in {-1, 0, 1}, scores in [-49, 49]; the
    aux_weight rows cycle through (1,1), (1,0), (0,1), (0,0), or with reply_weights=False through (1,0), (0,0): no sample has a
    reply, so that loss's denominator is the clamp.  float32 arrays, as the trainer's."""
    f32 = np.float32
    cells = rng.integers(0, 4, size=(n, 7, 7))
    feats = np.stack([np.ones_like(cells), cells == 1, cells == 2, cells == 3], axis=3).astype(f32)

    def dirichlet_rows():
        rows = np.zeros((n, 833), dtype=np.float64)
        for row in rows:
            at = rng.choice(833, size=int(rng.integers(1, 40)), replace=False)
            row[at] = rng.dirichlet(np.ones(len(at)))
        return rows.reshape(n, 7, 7, 17).astype(f32)

    values = np.where(rng.random(n) < 0.5, rng.choice([-1.0, 1.0], size=n), rng.uniform(-1, 1, size=n)).astype(f32)[:, None]
    batch = feats, dirichlet_rows(), values
    if not aux:
        return batch
    ownership = rng.integers(-1, 2, size=(n, 7, 7)).astype(f32)
    score = rng.integers(-49, 50, size=(n, 1)).astype(f32)
    rows = [(1, 1), (1, 0), (0, 1), (0, 0)] if reply_weights else [(1, 0), (0, 0)]
    weight = np.array([rows[i % len(rows)] for i in range(n)], dtype=f32)
    reply = dirichlet_rows() * weight[:, 1][:, None, None, None]
    return batch + (ownership, score, reply, weight)


def _tensors(result):
    out = [("conv%d" % i, a) for i, a in enumerate(result["conv"])]
    if result.get("aux") is not None:
        out += [(k, result["aux"][k]) for k in AUX_KEYS]
    if result.get("affine") is not None:
        out += [("affine%d%s" % (i, "gb"[j]), a) for i, pair in enumerate(result["affine"]) for j, a in enumerate(pair)]
    return out


def distances(got, ref, start):
    """The distance of a result to a reference result, per quantity; results and `start` shaped as run's return value
    ("losses" optional in `got`, absent from `start`).
    -> {"update": over all trainable tensors the worst max|dw_got - dw_ref| / max|dw_ref|, dw = w_after - w_before;
        "statistics": max absolute difference of the moving statistics;
        "losses": worst relative difference of a loss term (None without losses in `got`);  "worst": which tensor}"""
    update, worst = 0.0, None
    for (name, a), (_, b), (_, s) in zip(_tensors(got), _tensors(ref), _tensors(start)):
        a, b, s = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (a, b, s))
        err = float(np.abs((a - s) - (b - s)).max() / np.abs(b - s).max())
        if not err <= update:                                              # (a NaN is the worst)
            update, worst = err, name
    apart = np.concatenate([np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) for a, b in zip(got["bn"], ref["bn"])])
    stats = float("nan") if np.isnan(apart).any() else float(apart.max())
    losses = None
    if got.get("losses") is not None:
        g, r = np.asarray(got["losses"], dtype=np.float64), np.asarray(ref["losses"], dtype=np.float64)
        assert g.shape == r.shape
        rel = np.abs(g - r) / np.where(r == 0.0, 1.0, np.abs(r))           # (a term that is exactly zero: absolute)
        losses = float("nan") if np.isnan(rel).any() else float(rel.max())
    return {"update": update, "statistics": stats, "losses": losses, "worst": worst}


def kink_margin(result, again):
    """How far the nearest ReLU input of `result` (float64) lies from zero, against the noise a float32 run puts on such an input.
    -> (min |x| over every ReLU input of every step, the largest per-layer root mean square of x_again - x_result), `again` the
    float32 run of the same steps.  A ReLU input within the noise of zero may fall on either side of it in two float32 runs,
    and the one that crosses switches a whole path of the gradient on or off — an update error of a per cent, four orders
    above rounding — so an allowance made of rounding distances means something only where the margin is many times the noise."""
    margin, noise = float("inf"), 0.0
    for step, step_again in zip(result["relu_inputs"], again["relu_inputs"]):
        for x, y in zip(step, step_again):
            margin = min(margin, float(np.abs(x).min()))
            noise = max(noise, float(np.sqrt(np.mean((np.asarray(y, dtype=np.float64) - x) ** 2))))
    return margin, noise
