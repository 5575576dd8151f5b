#!/usr/bin/python
"""Rates of the device alpha-beta search (profiles/alphabeta.txt): roots/s and nodes/s of azh_alphabeta_search at depths
1 .. 4 on mid-game roots of uniform-random games (plies 20 .. 60), the pruning ratio against the host's plain negamax on a
sample of them, and teacher games/s of azh_alphabeta_play with and without the Python entry builder.

Every time is the wall clock of the whole call — allocation, copies in and out, the launch — as a caller sees it: the
median of `--reps` calls after one untimed call."""
import argparse
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from ataxxzero_amd import link, selfplay, supervised  # noqa: E402


def midgame_roots(n, seed):
    x, o, bl, turn = selfplay.parse_fen(selfplay.START_FEN_PLAIN)
    plies, _, boards, _ = link.random_play(512, seed, x, o, bl, turn, 400)
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        g = int(rng.integers(512))
        p = int(rng.integers(20, 61))
        if p < plies[g]:
            out.append([int(boards[g, p, 0]) | ((p & 1) << 63), int(boards[g, p, 1])])
    return np.array(out, dtype=np.uint64)


def timed(call, reps):
    call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget", type=int, default=1 << 20, help="node budget of the depths past 3")
    ap.add_argument("--plain-sample", type=int, default=64, help="roots the host's plain negamax counts (depths 1 .. 3)")
    ap.add_argument("--teacher-games", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    link.require_gpu()
    roots = midgame_roots(args.roots, args.seed)
    print("azh_alphabeta_search, %d mid-game roots (plies 20 .. 60 of uniform-random games), median of %d calls"
          % (len(roots), args.reps))
    for depth in (1, 2, 3, 4):
        budget = 0 if depth <= link.ALPHABETA_UNBOUNDED_DEPTH else args.budget
        sec, out = timed(lambda: link.alphabeta_search(roots, 0, depth, budget), args.reps)
        nodes = int(out.nodes.sum())
        print("  depth %d budget %-8d %9.3f ms  %10.0f roots/s  %8.1f M nodes/s  %8.0f nodes/root  completed %.3f"
              % (depth, budget, sec * 1e3, len(roots) / sec, nodes / sec / 1e6, nodes / len(roots),
                 float((out.depth_done == depth).mean())))
    sample = roots[:args.plain_sample]
    print("pruning: device nodes / plain negamax nodes (azh_alphabeta_host) on %d of the roots" % len(sample))
    for depth in (1, 2, 3):
        dev = int(link.alphabeta_search(sample, 0, depth).nodes.sum())
        plain = sum(link.alphabeta_host(int(b[0]) & ((1 << 63) - 1), int(b[1]), 0, int(b[0]) >> 63, depth)[3] for b in sample)
        print("  depth %d  device %10d  plain %12d  ratio %.4f" % (depth, dev, plain, dev / plain))
    x, o, bl, turn = selfplay.parse_fen(selfplay.START_FEN_PLAIN)
    thresholds = link.teacher_thresholds(supervised.OPENING_RANDOMIZATION_SCHEDULE)
    print("teacher games, %d per call, 400 plies at most, the reference's opening randomisation" % args.teacher_games)
    for depth in (1, 2, 3):
        sec, out = timed(lambda: link.alphabeta_play(args.teacher_games, args.seed, x, o, bl, turn, depth, 0, thresholds, 400), 1)
        t0 = time.perf_counter()
        entries = supervised.alphabeta_entries(args.teacher_games, args.seed, depth)
        whole = time.perf_counter() - t0
        print("  depth %d  azh_alphabeta_play %8.3f s = %8.1f games/s (mean %.1f plies, %d unfinished);  with the entry builder "
              "%8.3f s = %8.1f games/s" % (depth, sec, args.teacher_games / sec, float(out[0].mean()), int((out[1] == 0).sum()),
                                             whole, len(entries) / whole))


if __name__ == "__main__":
    main()
