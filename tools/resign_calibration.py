#!/usr/bin/python
"""Choose a resign threshold from games that carry the search's value at every ply.

    python tools/resign_calibration.py GAMES.json [GAMES.json ...] [--thresholds V,V,...] [--plies K,K,...]

Reads JSON-lines game files written by accelerated_generate_games.py with --record-values (or with a resign threshold: the
games that were resigned are left out, the play-through games and the ones the rule never fired in are used).  The resign
rule is a pure function of a line — "values", "full" where the playout cap was on, and the ply's parity (x moves on even
plies) — so it is replayed here for a grid of thresholds V (the value scale [-1, 1) of --resign-threshold) and run lengths
K (--resign-plies).  Per (V, K): the share of the games the rule would end, the share of THOSE in which the side that would
have resigned went on not to lose (the false positives), and the share of all plies that would not have been played.
"""
import argparse
import json
import sys

import numpy as np

THRESHOLDS = [-0.99, -0.98, -0.97, -0.95, -0.93, -0.9, -0.85, -0.8, -0.7, -0.6, -0.5]
PLIES = [1, 2, 3, 4]


def would_resign(entry, threshold, plies):
    """-> the ply at which the rule fires first in `entry` (the record of a resigned game would end with it), or None.
    The engine compares q = W / n in f32 with q_below = (V + 1) / 2 in f32; a line holds 2 q - 1 exactly, so q is
    recovered exactly."""
    q_below = np.float32((threshold + 1.0) / 2.0)
    full = entry.get("full")
    count = [0, 0]
    for p, v in enumerate(entry["values"]):
        if full is not None and not full[p]:
            continue                                  # a FAST ply neither advances nor resets a counter
        side = p % 2
        count[side] = count[side] + 1 if np.float32((v + 1.0) / 2.0) < q_below else 0
        if count[side] >= plies:
            return p
    return None


def calibrate(entries, thresholds=THRESHOLDS, plies=PLIES):
    """-> (games used, plies in them, [(V, K, games ended, of those not lost by the resigner, plies saved)])"""
    used = [e for e in entries if "values" in e and "resigned" not in e]
    total_plies = sum(len(e["values"]) for e in used)
    rows = []
    for k in plies:
        for v in thresholds:
            ended = wrong = saved = 0
            for e in used:
                p = would_resign(e, v, k)
                if p is None:
                    continue
                ended += 1
                resigner = 1 + p % 2
                wrong += int(e["result"] != 3 - resigner)
                saved += len(e["values"]) - (p + 1)
            rows.append((v, k, ended, wrong, saved))
    return len(used), total_plies, rows


def load(paths):
    entries = []
    for path in paths:
        with open(path) as f:
            entries += [json.loads(line) for line in f if line.strip()]
    return entries


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("games", nargs="+", metavar="GAMES")
    ap.add_argument("--thresholds", default=",".join(str(v) for v in THRESHOLDS))
    ap.add_argument("--plies", default=",".join(str(k) for k in PLIES))
    args = ap.parse_args(argv)
    entries = load(args.games)
    n, total, rows = calibrate(entries, [float(v) for v in args.thresholds.split(",")],
                               [int(k) for k in args.plies.split(",")])
    print("%d lines, %d of them with values and not resigned, %d plies" % (len(entries), n, total))
    if n == 0:
        return 1
    print("%9s %5s %11s %9s %15s %9s %12s" % ("threshold", "plies", "games ended", "share", "resigner !lost", "share",
                                              "plies saved"))
    for v, k, ended, wrong, saved in rows:
        print("%9.3f %5d %11d %8.1f%% %15d %8.1f%% %11.1f%%" % (v, k, ended, 100.0 * ended / n, wrong,
                                                                100.0 * wrong / ended if ended else 0.0,
                                                                100.0 * saved / total if total else 0.0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
