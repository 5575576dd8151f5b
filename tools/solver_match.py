"""Match of the single-position search with the proof layer on against the same search with it off ("Proven
wins and losses"): same net, same visits, openings of random plies so that the games are endgames.

Every opening — the position after --opening-plies plies of a uniformly random game (azh_random_play), kept if the game is
still on there — is played twice, the solver's side once x and once o.  Both sides are uai.Searcher.genmove at --visits
visits, K = --parallel-leaves, a fresh tree per move; the net has random weights (--blocks x 128).  Reported: the solver
side's wins, losses and score, the moves it played, and the share of them it played as proven (win or loss).

HOW TO MEASURE: one game at a time on one position at a time is slow (200 games at 400 visits: a quarter of an hour).  Search
settings are compared inside the device-resident loop by tools/settings_match.py, thousands of games in flight, with --solver
for both sides; the solver itself is one switch for both sides there, so solver on against off stays this tool's.

    python tools/solver_match.py [--games 200] [--visits 400] [--opening-plies 60] [--out profiles/FILE.txt]
"""
import argparse
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ataxxzero_amd import link, model, uai  # noqa: E402


def openings(count, plies, seed):
    """`count` unfinished positions after `plies` random plies from the start position."""
    start = uai.Position.initial()
    out, batch = [], 0
    while len(out) < count and batch < 64:
        n_plies, results, boards, moves = link.random_play(4 * count, seed + batch, start.x, start.o, 0, start.turn,
                                                           max_plies=400, trace=True)
        batch += 1
        for g in range(len(n_plies)):
            if n_plies[g] <= plies + 1 or len(out) >= count:
                continue
            # replay the moves on the host's own bookkeeping: the side to move comes out of the rules, not of a parity
            pos = uai.Position.initial()
            for mv in moves[g, :plies]:
                pos.move(int(mv))
            legal, result = pos.legal_moves()
            if result == 0 and legal:
                out.append((pos.x, pos.o, pos.turn))
    return out


def play(pos, sides, visits, max_plies=300):
    """-> (result 0 / 1 / 2, moves played by side 0's searcher, of which proven)."""
    played = proven = 0
    for _ in range(max_plies):
        legal, result = pos.legal_moves()
        if result != 0:
            return result, played, proven
        searcher = sides[pos.turn]
        mv = searcher.genmove(pos, visits=visits)
        if searcher.solver:
            played += 1
            proven += int(searcher.last_proven is not None)
        pos.move(mv)
    return 0, played, proven


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=200)
    ap.add_argument("--visits", type=int, default=400)
    ap.add_argument("--opening-plies", type=int, default=60)
    ap.add_argument("--parallel-leaves", type=int, default=1)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    link.require_gpu()
    random.seed(a.seed)
    conv, bn = model.random_init(a.blocks, 128, seed=a.seed, perturb_bn=True)
    path = os.path.join(tempfile.mkdtemp(), "net.npy")
    model.save_model(path, conv, bn)
    on = uai.Searcher(path, dtype="f16", parallel_leaves=a.parallel_leaves, solver=True)
    off = uai.Searcher(path, dtype="f16", parallel_leaves=a.parallel_leaves, solver=False)
    start = time.time()
    wins = losses = unfinished = played = proven = games = 0
    lines = ["# tools/solver_match.py: solver on against off, %d visits, K = %d, %dx128 net with random weights, f16, openings of %d "
             "random plies, each played with the solver's side as x and as o" % (a.visits, a.parallel_leaves, a.blocks, a.opening_plies)]
    for x, o, turn in openings((a.games + 1) // 2, a.opening_plies, a.seed):
        for solver_side in (0, 1):
            if games >= a.games:
                break
            sides = (on, off) if solver_side == 0 else (off, on)
            result, n, p = play(uai.Position(x, o, turn), sides, a.visits)
            games += 1
            played += n
            proven += p
            wins += int(result == 1 + solver_side)
            losses += int(result == 2 - solver_side)
            unfinished += int(result == 0)
            print("game %3d solver=%s result %d  solver moves %d proven %d" % (games, "xo"[solver_side], result, n, p), flush=True)
    decided = max(wins + losses, 1)
    lines.append("games %d: solver side won %d, lost %d, unfinished %d: score %.3f of the decided games; solver moves %d, played "
                 "as proven %d (%.1f %%); %.0f s" % (games, wins, losses, unfinished, wins / decided, played, proven,
                                                    100.0 * proven / max(played, 1), time.time() - start))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
