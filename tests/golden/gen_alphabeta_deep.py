#!/usr/bin/env python3
"""Generate tests/golden/alphabeta_deep.json.gz: roots on which a plain negamax of depth 8 is affordable, answered by this
repository's own memoised restatement (tests/alphabeta_memo.py).  From the repository's root:

    python tests/golden/gen_alphabeta_deep.py

Every root lives in a small region carved out of the 49 cells by walls (REGIONS: 3x3, 3x4, 2x6 and an L of 12 cells, not
always in a corner, so that the wall words differ between roots).  Three families:
  game      every unfinished position of seeded uniformly random games from several start layouts, either side moving first
  finished  the position each of those games ended in (no move, rule 1 at the root: the values +-1008 at depth 8)
  forced    for every value +-1000 .. +-1007 that random play did not give at depth 8, the first of a seeded series of
            random fillings of the 6x2 region that has it: a forced win or loss in exactly 8 - rem plies
Each root's entry holds its fen (walls as '-'), its wall mask, [move, value, plain negamax nodes] for d = 1 .. 8 and, beside
those, the nodes a textbook alpha-beta enters at each depth (alphabeta_memo.pruned_nodes); the file also lists the depth-8
values that occur.  tests/test_alphabeta_memo.py recomputes a fixed sample, so the file cannot
drift from the restatement, and no test imports this script.

Measured on one CPU core: this script 21 s (14 s before the textbook counts were added; 210 roots, the largest plain count
24.8 M nodes, at most some 620 k remembered entries per region); the test's sample, every fifth root and the forced ones to
depth 8 with the textbook counts, 10 s.  A 4x4 region would take minutes per game: the regions stay at 12 cells.
"""
import gzip
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import alphabeta_memo as am  # noqa: E402
from tests import rules_reference as rr  # noqa: E402

DEPTH = 8


def rect(f0, r0, w, h):
    return [f + 7 * r for r in range(r0, r0 + h) for f in range(f0, f0 + w)]


# name -> (live cells, start layouts [(x cells, o cells)]), cells as (file, rank)
def _region(cells, starts):
    return sorted(cells), [([f + 7 * r for f, r in xs], [f + 7 * r for f, r in os_]) for xs, os_ in starts]


REGIONS = {
    "3x3 centre": _region(rect(2, 3, 3, 3), [([(2, 3), (4, 5)], [(4, 3), (2, 5)]), ([(2, 3)], [(4, 5)]), ([(3, 3)], [(3, 5)])]),
    "3x3 corner": _region(rect(4, 0, 3, 3), [([(4, 0), (6, 2)], [(6, 0), (4, 2)]), ([(4, 2)], [(6, 0)])]),
    "3x4 corner": _region(rect(0, 0, 3, 4), [([(0, 0), (2, 3)], [(2, 0), (0, 3)]), ([(0, 0)], [(2, 3)])]),
    "4x3 inside": _region(rect(2, 2, 4, 3), [([(2, 2), (5, 4)], [(5, 2), (2, 4)]), ([(2, 4)], [(5, 2)])]),
    "6x2 top": _region(rect(1, 5, 6, 2), [([(1, 5), (6, 6)], [(6, 5), (1, 6)]), ([(1, 5)], [(6, 6)])]),
    "2x6 side": _region(rect(5, 0, 2, 6), [([(5, 0), (6, 5)], [(6, 0), (5, 5)]), ([(5, 5)], [(6, 0)])]),
    "L12": _region(rect(1, 1, 4, 2) + rect(1, 3, 2, 2), [([(1, 4), (4, 2)], [(4, 1), (2, 4)]), ([(1, 1)], [(4, 2)])]),
}
GAMES_PER_START_AND_SIDE = 1
FORCED_REGION = "6x2 top"


def walls_of(cells):
    return am.ALL & ~sum(1 << c for c in cells)


def start_board(region, layout, turn):
    cells, starts = REGIONS[region]
    xs, os_ = starts[layout]
    return rr.Board.from_masks(sum(1 << c for c in xs), sum(1 << c for c in os_), walls_of(cells), turn)


def random_game(seed, board):
    """-> (the unfinished positions of one game of uniformly random legal moves, the position it ended in)"""
    rng = random.Random(seed)
    line = []
    while rr.result(board) == 0:
        line.append(board)
        board = rr.make_move(board, rng.choice(rr.legal_moves(board)))
    return line, board


def entry(region, family, board):
    answers = [list(am.search(board, d)) for d in range(1, DEPTH + 1)]
    pruned = [am.pruned_nodes(board, d) if family != "finished" else 0 for d in range(1, DEPTH + 1)]
    return {"region": region, "family": family, "fen": board.fen(), "walls": board.masks()[2], "answers": answers,
            "pruned": pruned}


def forced(region, wanted, tries=4000):
    """the first of `tries` seeded random fillings of the region (1 to 9 cells left empty, the others x or o by a fair coin,
    the side to move alternating) that has each wanted depth-8 value and is not finished"""
    cells, _ = REGIONS[region]
    walls = walls_of(cells)
    rng = random.Random("forced/" + region)
    found = {}
    for n in range(tries):
        empty = set(rng.sample(cells, rng.randrange(1, 10)))
        x = o = 0
        for cell in cells:
            if cell not in empty:
                if rng.random() < 0.5:
                    x |= 1 << cell
                else:
                    o |= 1 << cell
        move, value, _ = am.search_masks(x, o, walls, n & 1, DEPTH)
        if move != am.NO_MOVE and value in wanted and value not in found:
            found[value] = rr.Board.from_masks(x, o, walls, n & 1)
            if len(found) == len(wanted):
                break
    return [found[v] for v in sorted(found)]


def main():
    t0 = time.time()
    roots = []
    for region, (cells, starts) in REGIONS.items():
        seen = set()
        for layout in range(len(starts)):
            for turn in (0, 1):
                for game in range(GAMES_PER_START_AND_SIDE):
                    seed = "%s/%d/%d/%d" % (region, layout, turn, game)
                    line, last = random_game(seed, start_board(region, layout, turn))
                    for family, boards in (("game", line), ("finished", [last])):
                        for b in boards:
                            if (b.fen(), family) not in seen:
                                seen.add((b.fen(), family))
                                roots.append(entry(region, family, b))
        print("%-11s %4d roots so far, %8d memo entries, %6.1f s" % (region, len(roots), am.entries(), time.time() - t0), flush=True)
        if region != FORCED_REGION:
            am.forget(walls_of(cells))
    live = {r["answers"][-1][1] for r in roots if r["family"] == "game"}
    wanted = {s * (am.WIN + rem) for s in (1, -1) for rem in range(DEPTH)} - live
    for b in forced(FORCED_REGION, wanted):
        roots.append(entry(FORCED_REGION, "forced", b))
    values = sorted({r["answers"][-1][1] for r in roots})
    out = {"depth": DEPTH, "regions": {name: {"cells": cells, "walls": walls_of(cells)} for name, (cells, _) in REGIONS.items()},
           "roots": roots, "values_at_depth_8": values}
    path = os.path.join(HERE, "alphabeta_deep.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("%d roots (%d game, %d finished, %d forced), largest plain count %d, values at depth 8: %s" % (
        len(roots), sum(r["family"] == "game" for r in roots), sum(r["family"] == "finished" for r in roots),
        sum(r["family"] == "forced" for r in roots), max(r["answers"][-1][2] for r in roots), values))
    print("%s: %d bytes, %.1f s" % (path, os.path.getsize(path), time.time() - t0))


if __name__ == "__main__":
    main()
