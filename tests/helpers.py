"""Shared helpers for the parity tests (no reference imports: /root/reference does not
exist on the GPU box; only tests/golden fixtures and the oracle are used)."""
import gzip
import json
import os

import numpy as np

from ataxxzero_amd import link
from oracle import oracle_lib as orc
from tests import rules_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BLOCK4_MASK = sum(1 << (x + 7 * (6 - y)) for x, y in [(3, 2), (2, 3), (4, 3), (3, 4)])


def load_gz(name):
    with gzip.open(os.path.join(GOLDEN, name)) as f:
        return json.loads(f.read())


def fixture_positions(limit=None):
    """[(packed board (2,) u64, blockers, record)] from both golden position files."""
    out = []
    for name, blockers in (("rules_noblock.json.gz", 0), ("rules_block4.json.gz", BLOCK4_MASK)):
        for rec in load_gz(name)[:limit]:
            p = orc.pos_from_fen(rec["fen"])
            packed = np.array([int(p.pieces[0]) | (p.turn << 63), int(p.pieces[1])], dtype=np.uint64)
            out.append((packed, blockers, rec))
    return out


def synthetic_evals(leaf_boards):
    """Deterministic pseudo-evaluator: f32 logits (G,833) and values (G,) from the leaf
    boards alone, so the GPU engine and the oracle can be fed identical bits."""
    lb = np.asarray(leaf_boards, dtype=np.uint64).reshape(-1, 2)
    a = (lb[:, 0] % np.uint64(1000003)).astype(np.int64)
    b = (lb[:, 1] % np.uint64(999983)).astype(np.int64)
    k = np.arange(833, dtype=np.int64)
    h = (a[:, None] * (k[None, :] + 1) + b[:, None] * (k[None, :] + 7) + 13 * k[None, :] * k[None, :]) % 4001
    logits = (h.astype(np.float32) / np.float32(1000.0)) - np.float32(2.0)
    values = (((a * 31 + b * 17) % 2001).astype(np.float32) / np.float32(1000.0)) - np.float32(1.0)
    return np.ascontiguousarray(logits, dtype=np.float32), np.ascontiguousarray(values, dtype=np.float32)


def replay_game_entry(entry, start_fen, blockers_mask=None):
    """Check a JSON game entry against the oracle rules; returns the final result."""
    p = orc.pos_from_fen(start_fen)
    if blockers_mask is not None:
        p.blockers = blockers_mask
    assert len(entry["boards"]) == len(entry["moves"])
    for i, (b, m) in enumerate(zip(entry["boards"], entry["moves"])):
        assert [int(v) for v in orc.board_cells(p)] == b, "board mismatch at ply %d" % i
        assert orc.result(p) == 0
        legal = [orc.move_string(x) for x in orc.movegen(p)]
        assert m in legal, (m, legal)
        if "dists" in entry:
            d = entry["dists"][i]
            # the ONE_RANDOM_MOVE ply may play a legal move the search never expanded
            assert m in d or entry.get("random_ply") == i
            assert abs(sum(d.values()) - 1.0) < 1e-9 and set(d) <= set(legal)
        c = orc.move_from_string(m)
        orc.lib().orc_makemove(p, c & 0xFF, c >> 8)
    return orc.result(p)


# strides coprime to 833 = 7 * 7 * 17: k -> (k * stride + offset) % 833 is a permutation of the policy indices
_STRIDES = np.array([s for s in range(2, 200) if s % 7 and s % 17], dtype=np.int64)


def synthetic_evals_distinct(leaf_boards):
    """Pure-function evaluator whose 833 logits are pairwise DISTINCT for every board (a board-dependent permutation
    of an arithmetic progression over [-3, 3)), so PUCT never meets two equal priors and the search is independent of
    any tie rule.  This is the evaluator injected into the reference's engine.py by tests/golden/gen_engine_fixtures.py
    and fed to the oracle / the HIP engine by the tests that replay those fixtures."""
    lb = np.asarray(leaf_boards, dtype=np.uint64).reshape(-1, 2)
    a = (lb[:, 0] % np.uint64(1000003)).astype(np.int64)
    b = (lb[:, 1] % np.uint64(999983)).astype(np.int64)
    off = (a * 31 + b * 17) % 833
    stride = _STRIDES[(a + 3 * b) % len(_STRIDES)]
    k = np.arange(833, dtype=np.int64)
    p = (k[None, :] * stride[:, None] + off[:, None]) % 833
    logits = p.astype(np.float32) * np.float32(6.0 / 833.0) - np.float32(3.0)
    values = (((a * 31 + b * 17) % 2001).astype(np.float32) / np.float32(1000.0)) - np.float32(1.0)
    return np.ascontiguousarray(logits, dtype=np.float32), np.ascontiguousarray(values, dtype=np.float32)


def leaf_boards_from_features(features):
    """(n,7,7,4) reference feature rows (engine.py:53-73) -> (n,2) u64 (mover, opponent), square = x + 7 * (6 - y)."""
    f = np.asarray(features).reshape(-1, 7, 7, 4)
    out = np.zeros((len(f), 2), dtype=np.uint64)
    for x in range(7):
        for y in range(7):
            sq = np.uint64(x + 7 * (6 - y))
            out[:, 0] |= (f[:, x, y, 1] != 0).astype(np.uint64) << sq
            out[:, 1] |= (f[:, x, y, 2] != 0).astype(np.uint64) << sq
    return out


def linear_evals(features):
    """Asymmetric pure-function evaluator on feature rows (used to pin the symmetry averaging of nn_evals.py:48-62):
    policy = features @ A, value = tanh(features @ b) with integer-built A, b (no RNG stream to drift)."""
    f = np.asarray(features, dtype=np.float64).reshape(-1, 196)
    i = np.arange(196, dtype=np.int64)[:, None]
    j = np.arange(833, dtype=np.int64)[None, :]
    A = (((i * 131 + j * 71 + i * j) % 257) - 128).astype(np.float64) / 128.0
    bvec = (((np.arange(196, dtype=np.int64) * 37) % 101) - 50).astype(np.float64) / 400.0
    return (f @ A).reshape(-1, 7, 7, 17), np.tanh(f @ bvec).reshape(-1, 1)


def random_line(fen, seed, blockers_mask=None):
    """One game of random legal moves from `fen` (numpy's PCG64 under `seed`; nine moves in ten a clone where there is one, so the
    board fills within some 60 plies): [(packed board (2,) u64 = x | turn << 63, o; ply; empty squares)] for every position of
    it that is not finished."""
    rng = np.random.default_rng(seed)
    p = orc.pos_from_fen(fen)
    if blockers_mask is not None:
        p.blockers = blockers_mask
    out = []
    while orc.result(p) == 0:
        x, o = int(p.pieces[0]), int(p.pieces[1])
        empty = 49 - bin(x).count("1") - bin(o).count("1") - bin(int(p.blockers)).count("1")
        out.append((np.array([x | (p.turn << 63), o], dtype=np.uint64), len(out), empty))
        moves = [int(m) for m in orc.movegen(p)]
        clones = [m for m in moves if (m & 0xFF) == (m >> 8)]
        if clones and rng.integers(10) != 0:
            moves = clones
        m = moves[int(rng.integers(len(moves)))]
        orc.lib().orc_makemove(p, m & 0xFF, m >> 8)
    return out


def cohort_positions(games, limit, fen=orc.START_FEN_SELFPLAY, seed=1, late_empty=4):
    """Positions and plies for set_positions under a game limit, one random line per slot, so that the games differ in length:
    the slots past the limit (g >= limit) stand late in their line, `late_empty` squares or fewer still empty — their games
    last a few plies; the cohort's slots alternate between an early position (ply 2 + g) and the middle of their line.
    -> boards (games, 2) u64, plies (games,) int32."""
    boards = np.zeros((games, 2), dtype=np.uint64)
    plies = np.zeros(games, dtype=np.int32)
    for g in range(games):
        line = random_line(fen, 1000 * seed + g)
        if g >= limit:
            pick = next((e for e in line if e[2] <= late_empty), line[-1])
        elif g % 2 == 0:
            pick = line[min(2 + g, len(line) - 1)]
        else:
            pick = line[len(line) // 2]
        boards[g], plies[g] = pick[0], pick[1]
    return boards, plies


# ---------------------------------------------------------------- evaluations that are not finite

NAN_POS_BITS, NAN_NEG_BITS = 0x7FC00001, 0xFFC00001     # quiet NaNs of both signs with a payload
_INF_BITS, _NEG_INF_BITS = 0x7F800000, 0xFF800000
_BIG_BITS = int(np.array([1e30], dtype=np.float32).view(np.uint32)[0])


def legal_policy_indices(leaf_board, blockers=0):
    """the policy indices of the mover's legal moves of a leaf board (mover, opponent), in move order"""
    p = orc.Pos()
    p.pieces[0], p.pieces[1], p.blockers, p.turn = int(leaf_board[0]), int(leaf_board[1]), int(blockers), 0
    return [int(orc.lib().orc_policy_index(int(m))) for m in orc.movegen(p)]


class HostileEvaluator:
    """A base evaluator overridden on a schedule the test controls: __call__(leaf_boards, keys) evaluates the boards with
    `base` and then, for every row i whose keys[i] is not None, applies the injections schedule(keys[i]) names — an iterable of
    (name, negative) — to that row's logits and value.  A key is whatever the harness knows of the row's slot before the step
    ((uid, ply, phase, root visits, ...)), so the engine and a restatement are fed identical bits and every phenomenon occurs by
    construction.  Bits are written as bits: a NaN is 0x7FC00001, or 0xFFC00001 where `negative`.  seen[(name, negative)]
    counts the injections into rows with counted[i] set (all rows by default).

        row_nan       every logit a NaN                     row_part_nan  logits 100 .. 299 a NaN
        row_inf3      +inf at every third logit             row_neginf    every logit -inf
        row_spike     1e30 at the last legal move's logit (every other prior underflows to zero)
        row_equal     every logit 0.25                      value_nan / value_pinf / value_ninf / value_plus1 / value_minus1
    """
    NAMES = ("row_nan", "row_part_nan", "row_inf3", "row_neginf", "row_spike", "row_equal",
             "value_nan", "value_pinf", "value_ninf", "value_plus1", "value_minus1")

    def __init__(self, schedule, base=synthetic_evals_distinct, blockers=0):
        self.schedule, self.base, self.blockers = schedule, base, blockers
        self.seen = {}

    def __call__(self, leaf_boards, keys, counted=None):
        lb = np.asarray(leaf_boards, dtype=np.uint64).reshape(-1, 2)
        logits, values = self.base(lb)
        lbits, vbits = logits.view(np.uint32), values.view(np.uint32)
        assert len(keys) == len(lb)
        for i, key in enumerate(keys):
            if key is None:
                continue
            for name, negative in self.schedule(key):
                nan = NAN_NEG_BITS if negative else NAN_POS_BITS
                if name == "row_nan":
                    lbits[i, :] = nan
                elif name == "row_part_nan":
                    lbits[i, 100:300] = nan
                elif name == "row_inf3":
                    lbits[i, ::3] = _INF_BITS
                elif name == "row_neginf":
                    lbits[i, :] = _NEG_INF_BITS
                elif name == "row_spike":
                    legal = legal_policy_indices(lb[i], self.blockers)
                    if legal:
                        lbits[i, legal[-1]] = _BIG_BITS
                elif name == "row_equal":
                    logits[i, :] = np.float32(0.25)
                elif name == "value_nan":
                    vbits[i] = nan
                elif name == "value_pinf":
                    vbits[i] = _INF_BITS
                elif name == "value_ninf":
                    vbits[i] = _NEG_INF_BITS
                elif name == "value_plus1":
                    values[i] = np.float32(1.0)
                elif name == "value_minus1":
                    values[i] = np.float32(-1.0)
                else:
                    raise ValueError(name)
                if counted is None or counted[i]:
                    self.seen[(name, bool(negative))] = self.seen.get((name, bool(negative)), 0) + 1
        return logits, values


def nonfinite_net(seed=3, cell=4, value_channels=(64,), policy_channel=58, policy_layer=16):
    """(conv, bn) of a one-block, 128-filter random net whose evaluations are not finite for some positions and finite for
    others.  The value head's 1x1 convolution keeps `value_channels` only, so a cell's activation is exactly 0 where those
    channels are, and the fc weight of `cell` is +inf: the value is a NaN where that cell's activation is 0 and +-1 elsewhere.
    The policy head's weight from input channel `policy_channel` to move layer `policy_layer` is +inf: that layer's logit of a
    cell is +inf where the channel is active there (every prior of a node with such a legal move is then zero) and a NaN where
    it is not; the other 16 layers stay finite.  The defaults were picked with oracle.net_oracle.forward over the positions of
    twelve random lines from the late start position of tests/engine_harness.py: about half of them get a NaN value,
    about half a +inf logit at a legal move (tests/test_hostile_net.py holds that)."""
    from ataxxzero_amd import model
    conv, bn = model.random_init(1, 128, seed=seed, perturb_bn=True)
    conv = [np.array(a, dtype=np.float32) for a in conv]
    keep = np.zeros(128, dtype=bool)
    keep[list(value_channels)] = True
    conv[4][0, 0, ~keep, 0] = 0.0
    conv[5][cell, 0] = np.inf
    conv[3][0, 0, policy_channel, policy_layer] = np.inf
    return conv, bn


BLOCK3_MASK = (1 << 0) | (1 << 9) | (1 << 33)


def orc_pos(b):
    p = orc.Pos()
    p.pieces[0], p.pieces[1], p.blockers = b.masks()
    p.turn = b.turn
    return p


def pocket_boards():
    """[(board, blockers mask)]: the side to move is walled in by blockers and its opponent has no stones, the boards on which
    the reference's two adjudication orders disagree (left out of rules_edge.json.gz for that reason)"""
    out = []
    for pocket in ([0], [48, 47], [6, 13], [42]):
        wall = {n for sq in pocket for n in rr.NEAR[sq] + rr.FAR[sq]} - set(pocket)
        for turn in (0, 1):
            cells = [rr.BLOCK if sq in wall else rr.EMPTY for sq in range(49)]
            for sq in pocket:
                cells[sq] = rr.X if turn == 0 else rr.O
            out.append((rr.Board(cells, turn), sum(1 << sq for sq in wall)))
    return out


def note(text):
    """numbers a green run should leave behind (pytest -q swallows prints): appended to gpurun_out/nn_gate.txt"""
    import os
    print(text)
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/nn_gate.txt", "a") as f:
        f.write(text + "\n")


def sample_leaf_boards(n, seed, blockers):
    p = orc.pos_from_fen(orc.START_FEN_PLAIN)
    plies, results, boards, moves = link.random_play(64, seed, p.pieces[0], p.pieces[1], blockers, 0, 300)
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        g = int(rng.integers(0, 64))
        ply = int(rng.integers(0, max(plies[g], 1)))
        x, o = int(boards[g, ply, 0]), int(boards[g, ply, 1])
        out.append([x, o] if ply % 2 == 0 else [o, x])
    return np.array(out, dtype=np.uint64)
