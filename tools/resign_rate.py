#!/usr/bin/python
"""What recording the search value and resigning cost and buy the generator: its own loop (two half-batches, evaluation
cache, select budget 48, bf16 tower, steady-state positions loaded as bench.py does) with the mode off, with values recorded
(q_below 0: no game resigns) and with resignation on, legs alternating in one process.  Per leg: plies/s, finished games/s,
evaluations/s, iterations/s, plies per finished game and the four resign counts.

    python tools/resign_rate.py [--network NPY] [--threshold V] [--plies K] [--playthrough F] [--pairs 3] [--out FILE]

Without --network the net is the random 12x128 one of the other rate tools: its values hover around 0, so its resign leg
measures the machinery and says nothing about a threshold.  Calibrate on a trained net: write games with
accelerated_generate_games.py --record-values, choose V with tools/resign_calibration.py, pass both here.
Appends its report to --out.  GPU box, repo root."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ataxxzero_amd import link, model, selfplay  # noqa: E402

SNAPSHOT = os.path.join(ROOT, "profiles", "round2_steady_state_positions.npz")


def leg(conv, bn, args, resign, seed):
    sp = selfplay.SelfPlay(conv, bn, games=args.games, visits=args.visits, dtype=args.dtype, seed=seed, streams=2,
                           flags=link.FLAG_EVAL_CACHE, select_budget=48, resign=resign)
    snap = np.load(SNAPSHOT)
    rng = np.random.default_rng(seed)
    n = len(snap["plies"])
    pick = rng.permutation(n) if args.games == n else rng.integers(0, n, size=args.games)
    sp.set_positions(snap["boards"][pick], snap["plies"][pick])
    for _ in range(args.fill // 250):
        sp.run(250)
        sp.drain()
    sp.sync()
    st0, rs0 = sp.stats(), sp.resign_stats()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sp.run(250)
        sp.fetch()
        sp.drain()
    sp.sync()
    dt = time.perf_counter() - t0
    st = {k: v - st0[k] for k, v in sp.stats().items()}
    rs = {k: v - rs0[k] for k, v in sp.resign_stats().items()}
    sp.close()
    return {"plies_s": st["plies"] / dt, "games_s": st["games"] / dt, "evals_s": st["nn_evals"] / dt,
            "iter_s": 250 * args.steps / dt, "plies_per_game": st["plies"] / max(1, st["games"]), "resign": rs}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--network", help=".npy weights (default: the random 12x128 net, seed 1)")
    ap.add_argument("--threshold", type=float, default=-0.9, help="resign threshold V on the value scale [-1, 1)")
    ap.add_argument("--plies", type=int, default=2)
    ap.add_argument("--playthrough", type=float, default=0.1)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--visits", type=int, default=400)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8, help="timed steps of 250 iterations per leg")
    ap.add_argument("--fill", type=int, default=1000, help="untimed iterations after the positions are loaded")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resign.txt"))
    args = ap.parse_args()
    selfplay.select_device(0)
    conv, bn = model.load_model(args.network) if args.network else model.random_init(12, 128, seed=1, perturb_bn=True)
    legs = [("off", None), ("record", (0.0, 1, 0.0)),
            ("resign", ((args.threshold + 1.0) / 2.0, args.plies, args.playthrough))]
    lines = ["== tools/resign_rate.py: MEASURED ON THE DEVICE (%s) — %d games in two half-batches, %s, %s, visits %d; resign = "
             "--resign-threshold %g --resign-plies %d --resign-playthrough %g; %d timed steps of 250 iterations per leg after "
             "%d untimed" % (link.pci_bus_id(0), args.games, args.network or "random 12x128 net", args.dtype, args.visits,
                             args.threshold, args.plies, args.playthrough, args.steps, args.fill)]
    rows = {name: [] for name, _ in legs}
    for pair in range(args.pairs):
        for name, resign in legs:
            r = leg(conv, bn, args, resign, seed=1000 + pair)
            rows[name].append(r)
            lines.append("%-6s plies/s %8.1f  games/s %7.2f  evals/s %9.0f  iterations/s %7.1f  plies per finished game %6.1f  "
                         "resigned %d, play-through %d, of those fired %d, of those not lost %d" % (
                             name, r["plies_s"], r["games_s"], r["evals_s"], r["iter_s"], r["plies_per_game"],
                             r["resign"]["resigned"], r["resign"]["playthrough"], r["resign"]["playthrough_fired"],
                             r["resign"]["playthrough_false"]))
            print(lines[-1], flush=True)
    for key, what in (("plies_s", "plies/s"), ("games_s", "finished games/s"), ("evals_s", "evaluations/s"),
                      ("iter_s", "iterations/s")):
        off = [r[key] for r in rows["off"]]
        lines.append("mean %-17s off %10.2f (%.2f .. %.2f)  record %10.2f (%+.2f %%)  resign %10.2f (%+.2f %%)" % (
            what, statistics.mean(off), min(off), max(off),
            statistics.mean(r[key] for r in rows["record"]),
            100.0 * (statistics.mean(r[key] for r in rows["record"]) / statistics.mean(off) - 1.0),
            statistics.mean(r[key] for r in rows["resign"]),
            100.0 * (statistics.mean(r[key] for r in rows["resign"]) / statistics.mean(off) - 1.0)))
        print(lines[-1])
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
