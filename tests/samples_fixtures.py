"""Records and draws built by hand for the sample store's tests: ring records with board moves only, the device's draw restated
on the oracle's Philox, and a mirror of games with and without a drawable ply."""
import ctypes

import numpy as np

from ataxxzero_amd import link
from ataxxzero_amd.link import RECORD_MAGIC as MAGIC
from oracle import oracle_lib as orc

STREAM_SAMPLE_DRAW = 8
PASS, FULL, BAD = link.SAMPLES_PLY_PASS, link.SAMPLES_PLY_FULL, link.SAMPLES_PLY_BAD
HAS_FULL, HAS_VALUES = link.SAMPLES_GAME_HAS_FULL, link.SAMPLES_GAME_HAS_VALUES

# every move of the board as (from, to) squares, square = file + 7 * rank: 49 clones and the jumps over a distance of two
MOVES = [(a, b) for a in range(49) for b in range(49)
         if a == b or max(abs(a % 7 - b % 7), abs(a // 7 - b // 7)) == 2]


def _bits(q):
    return int(np.array([q], dtype=np.float32).view(np.uint32)[0])


def random_record(rng, plies, counts_hi, kind=0, random_ply=None, result=1, zero_total_at=None, empty_at=None, uid=0):
    """Record words as the device loop leaves them in its ring (the idea of tests/record_fixtures.py::random_record, with
    board moves only — a trainer must be able to read the line — and the kind bits 4, 16 and 32)."""
    words = [MAGIC, 3, uid, plies, result, 0, 0 if random_ply is None else random_ply + 1, kind]
    for p in range(plies):
        cells = rng.integers(0, 3, size=49)
        x = sum(1 << i for i in range(49) if cells[i] == 1)
        o = sum(1 << i for i in range(49) if cells[i] == 2)
        nd = 0 if empty_at == p else int(rng.integers(1, 40))
        chosen = [MOVES[j] for j in rng.choice(len(MOVES), size=nd, replace=False)]
        counts = [int(v) for v in rng.integers(0, counts_hi + 1, size=nd)]
        if zero_total_at == p:
            counts = [0] * nd
        frm, to = chosen[0] if chosen else MOVES[int(rng.integers(len(MOVES)))]
        word5 = int(rng.integers(0, 2)) if kind & 4 else 0
        if kind & 16:
            q = [np.nan, np.inf, -np.inf, 0.5, 1.0, 0.0, float(rng.random())][int(rng.integers(0, 7))]
            word5 = (_bits(q) & 0x7FFFFFFF) | (word5 << 31)
        words += [x & 0xFFFFFFFF, x >> 32, o & 0xFFFFFFFF, o >> 32, (frm | to << 8) | nd << 16, word5]
        words += [(f | t << 8) | c << 16 for (f, t), c in zip(chosen, counts)]
    words[5] = len(words)
    return np.array(words, dtype=np.uint32)


def marker(uid):
    return np.array([MAGIC, 0, uid, 0, 0, 8, 0, 1], dtype=np.uint32)


def _arrays_equal(a, b):
    for name in link.SampleArrays.__slots__:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert x.tobytes() == y.tobytes(), name      # bit for bit: f32 weights, f64 values


def philox(seed, c0, c1, c2, c3):
    out = (ctypes.c_uint32 * 4)()
    orc.lib().orc_probe_philox(seed, c0, c1, c2, c3, out)
    return [int(v) for v in out]


def restated_draw(seed, step, i, first_game, n_games, games, flags):
    for a in range(64):
        v = philox(seed, step, i, a, STREAM_SAMPLE_DRAW)
        g = first_game + (v[0] * n_games >> 32)
        first, plies, word, random_ply_1 = (int(w) for w in games[g])
        candidates = [p for p in range(plies) if not word & HAS_FULL or flags[first + p] & FULL]
        if not candidates:
            continue
        ply = random_ply_1 if random_ply_1 else candidates[v[1] * len(candidates) >> 32]
        if ply >= plies or flags[first + ply] & (PASS | BAD):
            continue
        return g, ply, v[2] >> 29, a + 1
    return -1, -1, -1, 64


def draw_mirror():
    """40 games, exactly half of which can never give a sample."""
    rng = np.random.default_rng(40)
    games, flags = [], []

    def add(ply_flags, word=1, random_ply_1=0):
        games.append((len(flags), len(ply_flags), word, random_ply_1))
        flags.extend(ply_flags)

    undrawable = [
        lambda: add([0, 0, 0, 0], 1 | HAS_FULL),                            # "full" without one full ply
        lambda: add([0, 0, PASS, 0, 0], 2, 2),                              # the ply after the random move is a pass
        lambda: add([BAD] * 6),                                             # every ply bad
        lambda: add([PASS]),                                                # one ply, a pass
        lambda: add([FULL | BAD, 0, FULL | PASS, 0], 2 | HAS_FULL | HAS_VALUES),   # its full plies are bad or passes
        lambda: add([0, 0, 0], 1, 3),                                       # the random move was the last one
        lambda: add([0, 0, FULL], 1 | HAS_FULL, 1),                         # full plies, but random_ply + 1 is bad below
    ]
    drawable = [
        lambda: add([0] * int(rng.integers(2, 60)), 1 + int(rng.integers(2))),
        lambda: add([0]),                                                   # a one-ply game
        lambda: add([0, FULL, 0, FULL | BAD, FULL | PASS, FULL, 0], 1 | HAS_FULL),
        lambda: add([0, 0, 0, PASS, BAD], 2 | HAS_VALUES, 2),
        lambda: add([BAD, PASS, 0, BAD, PASS, BAD]),                        # one good ply among six
    ]
    order = [0] * 20 + [1] * 20
    rng.shuffle(order)
    for k, kind in enumerate(order):
        (drawable if kind else undrawable)[k % (5 if kind else 7)]()
        if not kind and k % 7 == 6:
            flags[games[-1][0] + 1] |= BAD
    games = np.array(games, dtype=np.uint32)
    flags = np.array(flags, dtype=np.uint8)
    can = []
    for first, plies, word, r1 in games.tolist():
        cand = [p for p in range(plies) if not word & HAS_FULL or flags[first + p] & FULL]
        plys = ([r1] if r1 else cand) if cand else []
        can.append(any(p < plies and not flags[first + p] & (PASS | BAD) for p in plys))
    assert sum(can) == 20 and len(can) == 40
    return games, flags, can
