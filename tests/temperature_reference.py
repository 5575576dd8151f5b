"""The per-ply temperature of the move played and of the root policy (azh_engine_set_temperature) restated in Python, for
the tests, from the definition in DESIGN.md ("Temperature of the move and of the root policy") and without the engine.

    the table: t(p) = final + (start - final) * 2 ** (-p / halflife) in float64 (halflife > 0, else start), final from the
        cutoff on, rounded to f32, values below 1/64 set to 0
    the weights of a root with visit counts n: T == 1 the counts themselves; T == 0 2^20 at the first maximum, 0 elsewhere;
        else q_j = min((u32)(expf(min(logf((f32)n_j) - logf((f32)n_max), 0) / T) * 2^20), 2^20) for n_j >= 1 and 0 for
        n_j == 0, every operation a single f32 one, expf and logf the oracle's deterministic ones
    the pick: S = sum q, r = (v0 * S) >> 32 with v0 word 0 of philox(seed; uid, ply, 1, 0) from the oracle, the first j in
        edge order with q_0 + ... + q_j > r (edge 0 where no edge weighs anything)
    the tempered root priors: priors_reference.priors on the row multiplied in f32 by np.float32(1) / np.float32(R)
"""
import ctypes

import numpy as np

from oracle import oracle_lib as orc
from tests import priors_reference

F32 = np.float32
ONE = 1 << 20
STREAM_SAMPLE = 1


def table(max_plies, start, final=None, halflife=0.0, cutoff=None):
    final = start if final is None else final
    out = np.zeros(max_plies, dtype=np.float32)
    for p in range(max_plies):
        t = final + (start - final) * 2.0 ** (-p / halflife) if halflife > 0 else float(start)
        if cutoff is not None and p >= cutoff:
            t = float(final)
        t = F32(t)
        out[p] = t if t >= F32(1.0 / 64.0) else F32(0.0)
    return out


def weights(visits, T):
    """-> the M weights as Python ints"""
    n = [int(v) for v in visits]
    T = F32(T)
    if T == F32(1.0):
        return n
    best = max(range(len(n)), key=lambda j: (n[j], -j))  # the first maximum
    if T == F32(0.0):
        return [ONE if j == best else 0 for j in range(len(n))]
    logf, expf = orc.lib().orc_probe_logf, orc.lib().orc_probe_expf
    lmax = F32(logf(float(F32(n[best]))))
    q = []
    for v in n:
        if v == 0:
            q.append(0)
            continue
        d = min(F32(F32(logf(float(F32(v)))) - lmax), F32(0.0))
        w = F32(expf(float(F32(d / T))))
        q.append(min(int(F32(w * F32(1048576.0))), ONE))
    return q


def v0_of(seed, uid, ply):
    out = (ctypes.c_uint32 * 4)()
    orc.lib().orc_probe_philox(int(seed), int(uid), int(ply), STREAM_SAMPLE, 0, out)
    return int(out[0])


def pick_from(q, v0):
    """the first j with q_0 + ... + q_j > (v0 * S) >> 32; 0 where nothing weighs"""
    r = (int(v0) * sum(q)) >> 32
    cum = 0
    for j, w in enumerate(q):
        cum += w
        if cum > r:
            return j
    return 0


def pick(visits, T, seed, uid, ply):
    """-> (edge, weights)"""
    q = weights(visits, T)
    return pick_from(q, v0_of(seed, uid, ply)), q


def tempered_priors(row, moves, R, **kw):
    """The prior bits of a noise ply's root under the root policy temperature R."""
    row = np.asarray(row, dtype=np.float32).reshape(833)
    if F32(R) != F32(1.0):
        row = (row * (F32(1) / F32(R))).astype(np.float32)
    return priors_reference.priors(row, moves, **kw)
