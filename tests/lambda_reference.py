"""The lambda-return of a stored game restated on Python floats (include/ataxxzero_hip.h, "lambda-returns as value targets"): the
third statement of the definition, beside azh_samples_value_returns_host and the kernel.  Nothing here imports the package.

For p = T - 1 down to 0:  next = z_p if p == T - 1 else -G_{p+1};  G_p = (1.0 - lambda) * v_p + lambda * next, four IEEE double
operations in that order; a proven ply's G_p is +-1.0 by the proof's sign, and the recursion goes on from it."""
import struct

import numpy as np


def z_of(result, ply):
    """+1 when the game's result is the mover of `ply` (x on even plies), else -1 — also for a game without a result"""
    return 1 if result == 1 + ply % 2 else -1


def returns(values, result, lam, proofs=None):
    """-> [G_0 .. G_{T-1}] as Python floats"""
    T = len(values)
    G = [None] * T
    for p in reversed(range(T)):
        nxt = float(z_of(result, p)) if p == T - 1 else -G[p + 1]
        a = 1.0 - lam
        b = a * float(values[p])
        c = lam * nxt
        G[p] = b + c
        if proofs is not None and int(proofs[p]) != 0:
            G[p] = 1.0 if int(proofs[p]) > 0 else -1.0
    return G


def bits(doubles):
    """the doubles as 64-bit integers: what "bit for bit" compares"""
    return [struct.unpack("<Q", struct.pack("<d", float(v)))[0] for v in doubles]


def as_f32(doubles):
    """(float)G_p: the value column of a minibatch"""
    return np.asarray([float(v) for v in doubles], dtype=np.float64).astype(np.float32)


T_CASES = (1, 2, 3, 64, 65, 129)
LAMBDAS = (0.0, 1.0, 0.5, 0.7, 0.9)


def proof_cases(T, rng):
    """None, and proofs at the last ply, the first ply and two adjacent plies (signs drawn), where the game has the room"""
    cases = [None]
    for where in ([T - 1], [0], [T // 2, T // 2 + 1] if T >= 3 else [0, T - 1]):
        proofs = [0] * T
        for p in where:
            proofs[p] = int(rng.choice([-1003, -1000, 1000, 1002]))
        cases.append(proofs)
    return cases
