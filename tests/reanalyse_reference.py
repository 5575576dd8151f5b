"""Reanalysis of stored plies (include/ataxxzero_hip.h, "reanalysis of stored plies"), restated in plain Python / numpy: the
policy target and the value a root report gives a stored ply, and root report records built by hand in every shape the kernels
treat differently."""
import numpy as np

from ataxxzero_amd import link, training

WORDS = link.ROOT_REPORT_WORDS
MAX_MOVES = link.MAX_MOVES
# every move of the board as from | to << 8, square = file + 7 * rank: 49 clones and the jumps over a distance of two
MOVES = [a | b << 8 for a in range(49) for b in range(49)
         if a == b or max(abs(a % 7 - b % 7), abs(a // 7 - b // 7)) == 2]


class Malformed(Exception):
    pass


def board_move(mv):
    frm, to = mv & 0xFF, mv >> 8
    return mv <= 0xFFFF and frm < 49 and to < 49 and (
        frm == to or max(abs(to % 7 - frm % 7), abs(to // 7 - frm // 7)) == 2)


def policy_index(mv):
    """flat index 119 to_x + 17 to_y + layer, (x, y) = (sq % 7, 6 - sq // 7): the layer of a jump from training.DELTA_LAYER"""
    frm, to = mv & 0xFF, mv >> 8
    fx, fy, tx, ty = frm % 7, 6 - frm // 7, to % 7, 6 - to // 7
    return 119 * tx + 17 * ty + (16 if frm == to else training.DELTA_LAYER[(tx - fx, ty - fy)])


def retarget(record):
    """One record -> (index (n,) u16, weight (n,) f32, value as a Python float); n == 0 and value 0.0: the ply stays as it
    was.  Malformed for a record the definition calls so."""
    record = np.asarray(record, dtype=np.uint32)
    m = int(record[1])
    if m > MAX_MOVES:
        raise Malformed("%d edges" % m)
    rows = record[4:4 + 4 * m].reshape(m, 4)
    moves, visits = [int(v) for v in rows[:, 0]], [int(v) for v in rows[:, 1]]
    if any(n > 0 and not board_move(mv) for mv, n in zip(moves, visits)):
        raise Malformed("a visited move that is no clone and no jump")
    total = sum(visits)                                           # Python integers: exact
    if total == 0 or int(record[3]) != 0:
        return np.zeros(0, np.uint16), np.zeros(0, np.float32), 0.0
    index = np.array([policy_index(mv) for mv, n in zip(moves, visits) if n > 0], dtype=np.uint16)
    weight = np.array([np.float32(np.float64(n) / np.float64(total)) for n in visits if n > 0], dtype=np.float32)
    best = visits.index(max(visits))                              # the first in edge order on a tie
    with np.errstate(all="ignore"):
        q = rows[best:best + 1, 2].copy().view(np.float32)[0] / np.float32(visits[best])      # one f32 division
    value = 2.0 * float(q) - 1.0 if np.isfinite(q) else 0.0
    return index, weight, value


def bits(w):
    return int(np.array([w], dtype=np.float32).view(np.uint32)[0])


def record(moves, visits, scores, result=0, priors=None):
    """A root report record of the edges given; the principal variation is left empty (no reader of these tests needs it)."""
    m = len(moves)
    out = np.zeros(WORDS, dtype=np.uint32)
    out[0], out[1], out[2], out[3] = min(sum(int(v) for v in visits), 0xFFFFFFFF), m, 0, result
    for j in range(min(m, MAX_MOVES)):
        out[4 + 4 * j:8 + 4 * j] = [moves[j], visits[j], bits(scores[j]), bits(priors[j] if priors is not None else 1.0 / m)]
    return out


def shaped_records(rng, count):
    """`count` well-formed records cycling through the shapes: M = 1, 63, 64, 65 and 256; a single visited edge; visited edges in
    the last 64-edge round only; ties for the most visited edge; total == 0; a finished root; M == 0; W = NaN and W = inf on the
    most visited edge; visit counts up to 65535 on 256 edges; ordinary roots in between.  -> (records (count, WORDS) u32, the
    shape's name per record)"""
    def edges(m):
        return [MOVES[j] for j in rng.choice(len(MOVES), size=m, replace=False)]

    def scores(visits):
        return [float(rng.random()) * v for v in visits]

    def plain(m, hi=40):
        visits = [int(v) for v in rng.integers(0, hi + 1, size=m)]
        visits[int(rng.integers(m))] = hi                       # (never all zero)
        return record(edges(m), visits, scores(visits))

    def single(m):
        visits = [0] * m
        visits[int(rng.integers(m))] = int(rng.integers(1, 500))
        return record(edges(m), visits, scores(visits))

    def last_round():
        visits = [0] * 192 + [int(v) for v in rng.integers(0, 9, size=64)]
        visits[255] = 9
        return record(edges(256), visits, scores(visits))

    def ties(m):
        visits = [int(v) for v in rng.integers(0, 7, size=m)]
        for j in rng.choice(m, size=min(m, 3), replace=False):
            visits[int(j)] = 7
        return record(edges(m), visits, [float(j + 1) for j in range(m)])     # a different W on every edge

    def zero_total(m):
        return record(edges(m), [0] * m, [0.0] * m)

    def finished(m):
        r = plain(m)
        r[3] = 1 + int(rng.integers(2))
        return r

    def odd_w(w, m=20):
        visits = [int(v) for v in rng.integers(1, 30, size=m)]
        best = int(rng.integers(m))
        visits[best] = 31
        s = scores(visits)
        s[best] = w
        return record(edges(m), visits, s)

    def heavy():
        visits = [int(v) for v in rng.integers(60000, 65536, size=256)]
        visits[int(rng.integers(256))] = 65535
        return record(edges(256), visits, scores(visits))

    shapes = [("M=1", lambda: plain(1)), ("M=63", lambda: plain(63)), ("M=64", lambda: plain(64)), ("M=65", lambda: plain(65)),
              ("M=256", lambda: plain(256)), ("single", lambda: single(int(rng.integers(2, 257)))), ("last round", last_round),
              ("ties", lambda: ties(int(rng.integers(3, 200)))), ("ties in round 2", lambda: ties(130)),
              ("total=0", lambda: zero_total(int(rng.integers(1, 100)))), ("finished", lambda: finished(30)),
              ("M=0", lambda: record([], [], [])), ("W=nan", lambda: odd_w(np.nan)), ("W=inf", lambda: odd_w(np.inf)),
              ("W=-inf", lambda: odd_w(-np.inf)), ("heavy", heavy), ("plain", lambda: plain(int(rng.integers(2, 120)), 400))]
    names = [shapes[k % len(shapes)][0] for k in range(count)]
    return np.stack([shapes[k % len(shapes)][1]() for k in range(count)]), names


def malformed_records(rng):
    """Records the definition refuses: a visited move off the board, one that is no jump, bits above the move, M beyond 256."""
    out = []
    for bad in (49 | 49 << 8, 0 | 3 << 8, 0 | 8 << 8, 0x10000 | MOVES[5], 0xFFFF):
        r = shaped_records(rng, 5)[0][2]                          # 64 edges
        j = int(np.flatnonzero(r[5:5 + 4 * 64:4])[-1])            # a visited edge
        r[4 + 4 * j] = bad
        out.append(r)
    r = shaped_records(rng, 5)[0][4]
    r[1] = MAX_MOVES + 1
    out.append(r)
    return out


def kl(old_index, old_weight, new_index, new_weight):
    """KL(old || new) of two sparse targets in float64; a cell the old target has and the new one lacks counts with the new
    weight floored at 1e-12 (training.reanalyse's figure)."""
    new = {}
    for i, w in zip(new_index, new_weight):
        new[int(i)] = new.get(int(i), 0.0) + float(w)
    old = {}
    for i, w in zip(old_index, old_weight):
        old[int(i)] = old.get(int(i), 0.0) + float(w)
    return sum(w * (np.log(w) - np.log(max(new.get(i, 0.0), 1e-12))) for i, w in old.items() if w > 0.0)
