"""Restatements for the policy surprise tests (tests/test_surprise_host.py, tests/surprise_gpu_checks.py): the surprise of a ply
in float64 numpy with the error bound of the f32 computation, the weighted draw in Python integers on the oracle's Philox, and
the mirrors a weighted draw reads, built from plain lists."""
import ctypes
import math

import numpy as np

from ataxxzero_amd import link
from oracle import oracle_lib as orc
from tests import helpers
from tests.detmath_sets import EXPF_ULP, LOGF_ULP

F32 = np.float32
U = 2.0 ** -24                 # the unit roundoff of f32: one rounded operation is off by at most U relative
ULP = 2.0 ** -23               # an ulp of an f32 result is at most this much of it
STREAM_SAMPLE_DRAW = 8
PASS, FULL, BAD = link.SAMPLES_PLY_PASS, link.SAMPLES_PLY_FULL, link.SAMPLES_PLY_BAD
HAS_FULL = link.SAMPLES_GAME_HAS_FULL


# ---------------------------------------------------------------- the surprise

def kl_reference(logits, legal, t_index, t_weight):
    """KL(target || softmax of the f32 logits over `legal`) in float64 -> (the stored value: 0 when negative, the targets with
    a positive weight that are not legal, the bound on |f32 computation - this| derived below).

    The bound, to first order in U (every step of azh_samples_surprise_host against its exact value; n legal moves, T targets,
    d_j = l_j - mx, p = the softmax, S = sum exp d_j in [1, n]):
      d_j is one subtraction:                 |dd_j| <= U |d_j|
      e_j = det_expf(d_j):                    relative EXPF_ULP ulp + |dd_j|; a term below -87 reads 0: exp(-87) absolute
      S over lanes (ceil(n / 64) - 1 adds) and the 6-level butterfly, positive terms: relative (ceil(n / 64) + 5) U
        => eS = EXPF_ULP ULP + (ceil(n / 64) + 5) U + U E_p|d| + n exp(-87)          (relative error of S)
      log S = det_logf(S):                    |dlogS| <= eS + LOGF_ULP ULP ln S
      lp_t = d_t - log S:                     |dlp_t| <= U |d_t| + |dlogS| + U |lp_t|
      x_t = det_logf(w_t) - lp_t:             |dx_t| <= LOGF_ULP ULP |ln w_t| + |dlp_t| + U |x_t|
      term_t = w_t x_t:                       |dterm_t| <= w_t |dx_t| + U |term_t|
      the sum of T terms of either sign:      (ceil(T / 64) + 5) U sum |term_t|
    and the whole is multiplied by 1.001 for the terms of second order (each at most a few hundred U of a first-order one).
    Setting a negative sum to 0 moves it towards the reference's value, which is clamped alike."""
    l = np.asarray(logits, dtype=np.float64)
    legal = np.asarray(legal, dtype=np.int64)
    t_index = np.asarray(t_index, dtype=np.int64)
    w = np.asarray(t_weight, dtype=np.float64)
    n = len(legal)
    mx = l[legal].max()
    d = l[legal] - mx
    e = np.exp(d)
    S = e.sum()
    p = e / S
    log_s = math.log(S)
    is_legal = np.zeros(833, dtype=bool)
    is_legal[legal] = True
    use = (w > 0) & is_legal[t_index]
    illegal = int(((w > 0) & ~is_legal[t_index]).sum())
    wt, dt = w[use], l[t_index[use]] - mx
    lp = dt - log_s
    x = np.log(wt) - lp
    term = wt * x
    kl = float(term.sum())
    e_s = EXPF_ULP * ULP + (math.ceil(n / 64) + 5) * U + U * float((p * np.abs(d)).sum()) + n * math.exp(-87.0)
    d_log_s = e_s + LOGF_ULP * ULP * log_s
    d_x = LOGF_ULP * ULP * np.abs(np.log(wt)) + (U * np.abs(dt) + d_log_s + U * np.abs(lp)) + U * np.abs(x)
    bound = float((wt * d_x).sum() + U * np.abs(term).sum() + (math.ceil(max(len(term), 1) / 64) + 5) * U * np.abs(term).sum())
    return max(kl, 0.0), illegal, 1.001 * bound


def mover_view(packed):
    """A fixture's packed board (x | turn << 63, o) -> (mover's stones, opponent's stones, turn)."""
    x, o, turn = int(packed[0]) & ((1 << 63) - 1), int(packed[1]), int(packed[0]) >> 63
    return (o, x, turn) if turn else (x, o, turn)


def fixture_views(limit=None):
    """[(mover, opponent, turn, legal policy indices from the rules oracle)] of the golden positions without blockers."""
    out = []
    for packed, blockers, _ in helpers.fixture_positions(limit):
        if not blockers:
            mover, opponent, turn = mover_view(packed)
            out.append((mover, opponent, turn, helpers.legal_policy_indices([mover, opponent])))
    return out


# ---------------------------------------------------------------- the weighted draw

def weight_units(w):
    """q = floor(w * 65536 + 0.5) of an f32 weight, in Python integers and fractions of two."""
    w = float(F32(w))
    return int(math.floor(w * 65536.0 + 0.5))      # (w * 65536 is exact in a double: a power of two)


def candidates_of(first, plies, word, flags):
    return [p for p in range(plies) if not word & HAS_FULL or flags[first + p] & FULL]


def build_mirror(specs):
    """specs: [(ply flags, game word, random_ply + 1, weights per ply or None)] -> games (G, 4) u32, flags (P,) u8, candidates
    (P,) u16, cum (P,) u32 as the store keeps them (None: every candidate weighs 65536)."""
    games, flags, cand, cum = [], [], [], []
    for ply_flags, word, r1, weights in specs:
        first = len(flags)
        games.append((first, len(ply_flags), word, r1))
        flags.extend(ply_flags)
        c = candidates_of(first, len(ply_flags), word, flags)
        total, run = 0, []
        for p in c:
            total += 65536 if weights is None else weight_units(weights[p])
            run.append(total)
        assert total < 1 << 32
        cand.extend(c + [0] * (len(ply_flags) - len(c)))
        cum.extend(run + [0] * (len(ply_flags) - len(c)))
    return (np.array(games, dtype=np.uint32).reshape(-1, 4), np.array(flags, dtype=np.uint8), np.array(cand, dtype=np.uint16),
            np.array(cum, dtype=np.uint32))


def philox(seed, c0, c1, c2, c3):
    out = (ctypes.c_uint32 * 4)()
    orc.lib().orc_probe_philox(seed, c0, c1, c2, c3, out)
    return [int(v) for v in out]


def restated_weighted_draw(seed, step, i, first_game, n_games, games, flags, candidate_lists, cums):
    """candidate_lists / cums: per game, plain lists (the game's candidates and the running sums of their units)."""
    for a in range(64):
        v = philox(seed, step, i, a, STREAM_SAMPLE_DRAW)
        g = first_game + (v[0] * n_games >> 32)
        first, plies, _, random_ply_1 = games[g]
        cand, cum = candidate_lists[g], cums[g]
        if not cand or cum[-1] == 0:
            continue
        R = v[1] * cum[-1] >> 32
        k = next(k for k, c in enumerate(cum) if c > R)          # the first k with cum[k] > R
        ply = random_ply_1 if random_ply_1 else cand[k]
        if ply >= plies or flags[first + ply] & (PASS | BAD):
            continue
        return g, ply, v[2] >> 29, a + 1
    return -1, -1, -1, 64


def per_game_lists(games, flags, cum):
    games = [tuple(int(v) for v in row) for row in games]
    flags = [int(f) for f in flags]
    lists = [candidates_of(first, plies, word, flags) for first, plies, word, _ in games]
    cums = [[int(c) for c in cum[first:first + len(c_list)]] for (first, _, _, _), c_list in zip(games, lists)]
    return games, flags, lists, cums


def edge_specs(rng):
    """The games of the issue's list; weights None: never given any."""
    long_w = rng.random(4096).astype(F32)
    long_w[rng.random(4096) < 0.3] = 0
    return [
        ([0], 1, 0, [2.5]),                                               # one candidate
        ([0, 0, 0, 0], 1 | HAS_FULL, 0, [1, 1, 1, 1]),                    # "full" without one full ply
        ([0, 0, 0], 2, 0, [0, 0, 0]),                                     # total 0
        ([0] * 9, 1, 0, [0, 1.5, 0, 0, 0.25, 3, 0, 0, 1e-6]),             # zeros on some plies (1e-6 rounds to 0 units)
        ([0, 0, 0, 0, 0], 2, 3, [5, 0, 0, 0, 1]),                         # random_ply: ply 3 whatever the weights say
        ([0] * 4096, 1, 0, long_w),                                       # the search's depth
        ([0, FULL, 0, FULL | BAD, FULL | PASS, FULL, 0], 1 | HAS_FULL, 0, [9, 0.5, 9, 4, 4, 2, 9]),
        ([0] * 12, 2, 0, None),                                           # never weighted
        ([BAD, PASS, 0, BAD, PASS, BAD], 1, 0, [0.125, 0.125, 3, 0.125, 0.125, 0.125]),   # one good ply among six, a heavy one
        ([0, 0, 0], 1, 0, [65535.0, 0.5, 0.25]),                          # a large total: 65535.75 * 65536 units
    ]
