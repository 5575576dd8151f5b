"""Match of the single-position search with first-play urgency and / or the growing exploration rate on against the same
search with the mode off ("First-play urgency and the exploration rate"): same net, same visits, the same
openings played twice with the colours swapped.

WITH RANDOM WEIGHTS THE POLICY IS FLAT AND THE VALUE IS NOISE: both knobs act through the priors and the mean scores of a
node, so a match of random nets says nothing about them.  Give a trained net with --network PATH (tools/learning_curve.py
writes one per generation); without it the tool plays --blocks x 128 random weights, which exercises the code path only.

Every opening — the position after --opening-plies plies of a uniformly random game (azh_random_play), kept if the game is
still on there — is played twice, the mode's side once x and once o.  Both sides are uai.Searcher.genmove at --visits visits,
K = --parallel-leaves, a fresh tree per move.  Reported: games, the mode's side's wins, losses and unfinished games, its score
of the decided games and the 95 % interval of that score (Wilson).

HOW TO MEASURE: this tool plays one game at a time on one position at a time, so 200 games at 400 visits take a quarter of
an hour and leave an interval of about +-7 points.  tools/settings_match.py plays the same comparison — and any other between
search settings — inside the device-resident loop, thousands of games in flight:
    python tools/settings_match.py --network model.npy --set visits=400 --set visits=400,fpu=0.25,cpuct-base=19652,cpuct-init=1.25

    python tools/exploration_match.py --network model.npy [--fpu-reduction 0.25] [--cpuct-base 19652 --cpuct-init 1.25]
                                      [--games 200] [--visits 400] [--opening-plies 8] [--out profiles/FILE.txt]
"""
import argparse
import math
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ataxxzero_amd import link, model, uai  # noqa: E402
from tools.solver_match import openings  # noqa: E402


def play(pos, sides, visits, max_plies=300):
    """-> result 0 (unfinished) / 1 (x won) / 2 (o won)."""
    for _ in range(max_plies):
        legal, result = pos.legal_moves()
        if result != 0:
            return result
        pos.move(sides[pos.turn].genmove(pos, visits=visits))
    return 0


def wilson(wins, n, z=1.96):
    """The 95 % interval of a share of `wins` in `n` decided games."""
    if n == 0:
        return 0.0, 1.0
    p = wins / n
    centre = (p + z * z / (2 * n)) / (1 + z * z / n)
    half = z * math.sqrt(p * (1 - p) / n + z * z / (4 * n * n)) / (1 + z * z / n)
    return centre - half, centre + half


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--network", default=None, metavar="PATH", help=".npy weights of a trained net (without it: random weights)")
    ap.add_argument("--fpu-reduction", type=float, default=0.25)
    ap.add_argument("--cpuct-base", type=float, default=19652.0)
    ap.add_argument("--cpuct-init", type=float, default=1.25)
    ap.add_argument("--no-fpu", action="store_true", help="leave first-play urgency off")
    ap.add_argument("--no-rate", action="store_true", help="leave the exploration rate constant")
    ap.add_argument("--games", type=int, default=200)
    ap.add_argument("--visits", type=int, default=400)
    ap.add_argument("--opening-plies", type=int, default=8)
    ap.add_argument("--parallel-leaves", type=int, default=1)
    ap.add_argument("--solver", action="store_true", help="both sides with the proof layer on")
    ap.add_argument("--blocks", type=int, default=2, help="depth of the random net (without --network)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.no_fpu and a.no_rate:
        ap.error("--no-fpu and --no-rate leave nothing to compare")
    link.require_gpu()
    random.seed(a.seed)
    path, net_text = a.network, a.network
    if path is None:
        conv, bn = model.random_init(a.blocks, 128, seed=a.seed, perturb_bn=True)
        path = os.path.join(tempfile.mkdtemp(), "net.npy")
        model.save_model(path, conv, bn)
        net_text = "%dx128 net with RANDOM weights (says nothing about the knobs)" % a.blocks
    knobs = dict(fpu_reduction=None if a.no_fpu else a.fpu_reduction, cpuct_base=None if a.no_rate else a.cpuct_base,
                 cpuct_init=a.cpuct_init)
    on = uai.Searcher(path, dtype="f16", parallel_leaves=a.parallel_leaves, solver=a.solver, **knobs)
    off = uai.Searcher(path, dtype="f16", parallel_leaves=a.parallel_leaves, solver=a.solver)
    start = time.time()
    wins = losses = unfinished = games = 0
    lines = ["# tools/exploration_match.py: exploration %s against off, %d visits, K = %d, solver %s, %s, f16, openings of %d random "
             "plies, each played with the mode's side as x and as o" % (on.exploration, a.visits, a.parallel_leaves,
                                                                        "on" if a.solver else "off", net_text, a.opening_plies)]
    for x, o, turn in openings((a.games + 1) // 2, a.opening_plies, a.seed):
        for side in (0, 1):
            if games >= a.games:
                break
            result = play(uai.Position(x, o, turn), (on, off) if side == 0 else (off, on), a.visits)
            games += 1
            wins += int(result == 1 + side)
            losses += int(result == 2 - side)
            unfinished += int(result == 0)
            print("game %3d mode=%s result %d" % (games, "xo"[side], result), flush=True)
    decided = wins + losses
    lo, hi = wilson(wins, decided)
    lines.append("games %d: the mode's side won %d, lost %d, unfinished %d: score %.3f of the decided games, 95 %% interval "
                 "%.3f .. %.3f; %.0f s" % (games, wins, losses, unfinished, wins / max(decided, 1), lo, hi, time.time() - start))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
