"""The positions the alpha-beta tests share (tests/test_alphabeta_host.py, tests/test_gpu_alphabeta.py) with the restatement's
answers (tests/alphabeta_reference.py), computed once per process and left unchanged.  The whole set stays under some
300 k restated nodes.  deep(): the roots of small walled regions with their answers to depth 8, read from the fixture."""
import collections
import random

from tests import alphabeta_reference as ab
from tests import rules_reference as rr
from tests.helpers import load_gz

START = "x5o/7/7/7/7/7/o5x x"
WALLED_START = "x5o/7/2-1-2/7/2-1-2/7/o5x x"
WIDE = "2oo1xx/o2o3/o2oooo/2oo2o/2oo3/o1oooo1/1o2o2 o"          # 157 moves, a forced win
LOST = "oxxxoxo/xoxxxxx/xoxxxxx/xxxxoxx/o1xxoox/xxxxxox/xxxxxxx o"  # 2 moves, a forced loss
FINISHED = ("xxxxxxx/xxxxxxx/xxxxxxx/xxxxxxx/ooooooo/ooooooo/ooooooo x", "7/7/7/3x3/7/7/7 o")  # a full board, no o stones
GAME_SEED = 20261020

_cache = {}


def random_game(seed, fen=START):
    """every position of one game of uniformly random legal moves that is not finished"""
    rng = random.Random(seed)
    b = rr.Board.from_fen(fen)
    line = []
    while rr.result(b) == 0:
        line.append(b)
        b = rr.make_move(b, rng.choice(rr.legal_moves(b)))
    return line


def cases():
    """[(name, board, depth the search is asked for)]: the depth is the greatest the case is restated at"""
    if "cases" not in _cache:
        out = [("start", rr.Board.from_fen(START), 3), ("walled start", rr.Board.from_fen(WALLED_START), 3),
               ("wide", rr.Board.from_fen(WIDE), 3), ("lost", rr.Board.from_fen(LOST), 3)]
        # the last ten positions of a random game, to depth 5 where one square is empty and to depth 4 where more are (a
        # plain negamax of depth 5 costs up to 190 k nodes on those; depth 4 at most 20 k)
        out += [("endgame %d" % i, b, 5 if b.count(rr.EMPTY) <= 1 else 4) for i, b in enumerate(random_game(GAME_SEED)[-10:])]
        # the widest move lists the hill climb finds (x to move, no o stones), with o on the first two empty squares
        walls = rr.Board.from_fen(WALLED_START).masks()[2]
        for name, seed, mask in (("hill climb 1", 1, 0), ("hill climb 2", 2, 0), ("hill climb walls", 3, walls)):
            b = rr.hill_climb(seed, blockers=mask, restarts=1)[1]
            for sq in [sq for sq in range(49) if b.cells[sq] == rr.EMPTY][:2]:
                b.cells[sq] = rr.O
            out.append((name, b, 2))
        _cache["cases"] = out
    return _cache["cases"]


def restated(name):
    """[(move, value, nodes of the iteration)] of a case for d = 1 .. its depth"""
    key = ("restated", name)
    if key not in _cache:
        board, depth = next((b, d) for n, b, d in cases() if n == name)
        _cache[key] = ab.all_depths(board, depth)
    return _cache[key]


def finished_boards():
    return [rr.Board.from_fen(f) for f in FINISHED]


Deep = collections.namedtuple("Deep", "board family region answers pruned")


def deep():
    """The roots of tests/golden/alphabeta_deep.json.gz (tests/golden/gen_alphabeta_deep.py: small walled regions, on which
    tests/alphabeta_memo.py restates depth 8) -> [Deep(board, "game" | "finished" | "forced", region name,
    [(move, value, plain negamax nodes of the iteration)] for d = 1 .. 8, [a textbook alpha-beta's nodes] for d = 1 .. 8)]"""
    if "deep" not in _cache:
        data = load_gz("alphabeta_deep.json.gz")
        _cache["deep"] = [Deep(rr.Board.from_fen(r["fen"]), r["family"], r["region"], [tuple(a) for a in r["answers"]],
                               r["pruned"]) for r in data["roots"]]
        assert all(d.board.masks()[2] == r["walls"] for d, r in zip(_cache["deep"], data["roots"]))
    return _cache["deep"]
