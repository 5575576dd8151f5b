"""Plain numpy / f32 restatement of the priors a node gets from one row of logits (apply_priors; DESIGN.md, "Search"
and "Leaf-parallel search"), written from the definition and without the engine.

    flags without PY_POSTERIOR: l = the row's logits gathered at the node's M legal moves, mx = max l,
        ex = exp(l - mx), S = the 64-lane sum of ex, P = ex / S (ex itself where S is not > 0)
    PY_POSTERIOR: mx over all 833 logits, S = the 64-lane sum of exp(row - mx) over all 833, ex = exp(l - mx) / S at the
        legal moves, P = ex / (64-lane sum of ex + 1e-6)
    root noise (weight w > 0): gm[j] = the game's gamma draw for edge j, T = the 64-lane sum of gm, and where T > 0
        P = w * (gm / T) + (1 - w) * P
    symmetry s != 0: the row holds the logits of the position's image; it is brought back first
        (symmetry_reference.logits_of_the_position), so every sum runs in the position's own index order.

The 64-lane sum: lane l adds the terms l, l + 64, ... in that order from 0, then the lanes are combined by the xor
butterfly with offsets 1, 2, 4, 8, 16, 32.  The exponential and the gamma draw are the oracle's probes (held bit for bit
against the device by test_detmath_bits_match_oracle); every other operation is an explicit np.float32 operation.  The result is
the priors' bit patterns with bit 31 cleared, as the edge records store them.
"""
import numpy as np

from oracle import oracle_lib as orc
from tests import symmetry_reference as sym

F32 = np.float32
FLAG_PY_POSTERIOR = 4


def expf(x):
    """exp of every element of an f32 array: the oracle's deterministic expf (0 for a NaN argument)."""
    f = orc.lib().orc_probe_expf
    x = np.asarray(x, dtype=np.float32)
    return np.array([f(float(v)) for v in x.reshape(-1)], dtype=np.float32).reshape(x.shape)


def wave_sum(v):
    """The 64-lane sum of an f32 vector: lane-striped partials from 0, then the xor butterfly 1, 2, 4, 8, 16, 32."""
    v = np.asarray(v, dtype=np.float32)
    rounds = (len(v) + 63) // 64
    padded = np.zeros(max(rounds, 1) * 64, dtype=np.float32)   # (x + 0 = x: a lane without a term in a round adds nothing)
    padded[:len(v)] = v
    lane = np.zeros(64, dtype=np.float32)
    for r in range(rounds):
        lane = (lane + padded[64 * r:64 * r + 64]).astype(np.float32)
    idx = np.arange(64)
    for off in (1, 2, 4, 8, 16, 32):
        lane = (lane + lane[idx ^ off]).astype(np.float32)
    return F32(lane[0])


def _max(v):
    """The largest element, NaN ignored (`if (v > mx) mx = v` from -inf)."""
    v = np.asarray(v, dtype=np.float32)
    v = v[~np.isnan(v)]
    return F32(v.max()) if len(v) else F32(-np.inf)


def priors(row, moves, flags=0, symmetry=0, noise=None):
    """The prior bits (M,) u32 of a node with the legal moves `moves` (u16 from | to << 8, in edge order) from the 833
    logits `row`.  symmetry: the symmetry under which the evaluator saw the position.  noise: None, or
    (alpha, weight, seed, uid, ply) for the root of a ply that gets the Dirichlet mix."""
    with np.errstate(all="ignore"):
        row = np.asarray(row, dtype=np.float32).reshape(833)
        if symmetry:
            row = sym.logits_of_the_position(row, symmetry)[0]
        idx = np.array([sym.policy_index(int(m)) for m in moves], dtype=np.int64)
        M = len(idx)
        l = row[idx] if M else np.zeros(0, np.float32)
        if flags & FLAG_PY_POSTERIOR:
            mx = _max(row)
            S = wave_sum(expf(row - mx))
            ex = (expf(l - mx) / S).astype(np.float32)
            den = F32(wave_sum(ex) + F32(1e-6))
            P = (ex / den).astype(np.float32)
        else:
            mx = _max(l)
            ex = expf(l - mx)
            S = wave_sum(ex)
            P = (ex / S).astype(np.float32) if S > 0 else ex
        if noise is not None and F32(noise[1]) > 0:
            alpha, weight, seed, uid, ply = noise
            gamma = orc.lib().orc_probe_gamma
            gm = np.array([gamma(float(F32(alpha)), int(seed), int(uid), int(ply), j) for j in range(M)], dtype=np.float32)
            T = wave_sum(gm)
            w = F32(weight)
            omw = F32(F32(1.0) - w)
            if T > 0:
                d = (gm / T).astype(np.float32)
                P = ((w * d).astype(np.float32) + (omw * P).astype(np.float32)).astype(np.float32)
        return np.ascontiguousarray(P, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
