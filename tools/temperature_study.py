#!/usr/bin/python
"""What the per-ply temperature of the move and of the root policy does to the generator's games and what it costs: its own
loop (two half-batches, evaluation cache, select budget 48, bf16 tower, games from the start position) for a fixed time per
leg with four schedules — off; AlphaZero's (1, then 0 from ply 30); KataGo's (0.8 -> 0.2, half-life 19); the latter with the
root policy at 1.25 -> 1.1 — legs alternating in one process.  Per leg: finished games/s, MCTS steps/s, iterations/s, the
share of plies whose move is not the most visited one by ply decile, the mean visit share of the move played, the mean game
length and, with --record-values, the share of plies after which the mover's next recorded value is lower by more than 0.3.

    python tools/temperature_study.py [--network NPY] [--seconds 40] [--rounds 2] [--record-values] [--out FILE]

The off leg runs the untouched kernels (the queued moves inside the tower launch); the on legs play their moves in the
move-playing launch of its own, the launch forced playouts pay for too (profiles/forced_playouts.txt).  Without --network the
net is the random 12x128 one of the other rate tools: its games say how the schedules sample, not how a trained net plays.
Appends its report to --out.  GPU box, repo root."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ataxxzero_amd import link, model, selfplay  # noqa: E402

SCHEDULES = [
    ("off", dict()),
    ("alphazero", dict(temperature=1.0, temperature_final=0.0, cutoff=30)),
    ("katago", dict(temperature=0.8, temperature_final=0.2, halflife=19.0)),
    ("katago+root", dict(temperature=0.8, temperature_final=0.2, halflife=19.0, root_policy_temperature=1.25,
                         root_policy_temperature_final=1.1)),
]
DECILES = 10


def game_figures(lines, acc):
    """the moves of finished games against their own dists (and values)"""
    for line in lines:
        entry = json.loads(line)
        acc["games"] += 1
        acc["plies"] += len(entry["moves"])
        values = entry.get("values")
        for ply, (move, dist) in enumerate(zip(entry["moves"], entry["dists"])):
            d = min(ply // 10, DECILES - 1)
            acc["decile_plies"][d] += 1
            acc["decile_not_best"][d] += int(dist[move] < max(dist.values()))
            acc["share"] += dist[move]
            if values is not None and ply + 2 < len(values):
                acc["value_pairs"] += 1
                acc["value_drops"] += int(values[ply + 2] < values[ply] - 0.3)


def leg(conv, bn, args, kwargs, seed):
    resign = (0.0, 1, 0.0) if args.record_values else None
    sp = selfplay.SelfPlay(conv, bn, games=args.games, visits=args.visits, dtype=args.dtype, seed=seed, streams=2,
                           flags=link.FLAG_EVAL_CACHE, select_budget=48, resign=resign,
                           temperature=selfplay.temperature_tables(400, **kwargs))
    acc = {"games": 0, "plies": 0, "share": 0.0, "value_pairs": 0, "value_drops": 0,
           "decile_plies": [0] * DECILES, "decile_not_best": [0] * DECILES}
    for _ in range(args.fill // 250):
        sp.run(250)
        sp.drain()
    sp.sync()
    st0 = sp.stats()
    t0 = time.perf_counter()
    iterations = 0
    while time.perf_counter() - t0 < args.seconds:
        sp.run(250)
        sp.fetch()
        game_figures(sp.drain(), acc)
        iterations += 250
    sp.sync()
    dt = time.perf_counter() - t0
    st = {k: v - st0[k] for k, v in sp.stats().items()}
    sp.close()
    acc.update(games_s=st["games"] / dt, steps_s=st["steps"] / dt, iter_s=iterations / dt, seconds=dt)
    return acc


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--network", help=".npy weights (default: the random 12x128 net, seed 1)")
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--visits", type=int, default=400)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--seconds", type=float, default=40.0, help="timed seconds per leg")
    ap.add_argument("--rounds", type=int, default=2, help="times the four legs are run, alternating")
    ap.add_argument("--fill", type=int, default=500, help="untimed iterations at the start of a leg")
    ap.add_argument("--record-values", action="store_true", help="record the search value in every leg, the off one too")
    ap.add_argument("--only", help="comma-separated schedule names (default: all four)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temperature.txt"))
    args = ap.parse_args()
    selfplay.select_device(0)
    conv, bn = model.load_model(args.network) if args.network else model.random_init(12, 128, seed=1, perturb_bn=True)
    schedules = [s for s in SCHEDULES if not args.only or s[0] in args.only.split(",")]
    lines = ["== tools/temperature_study.py: MEASURED ON THE DEVICE (%s) — %d games in two half-batches from the start position, "
             "%s, %s, visits %d%s; %g timed seconds per leg after %d untimed iterations" % (
                 link.pci_bus_id(0), args.games, args.network or "random 12x128 net", args.dtype, args.visits,
                 ", values recorded" if args.record_values else "", args.seconds, args.fill)]
    rows = {name: [] for name, _ in schedules}
    for rnd in range(args.rounds):
        for name, kwargs in schedules:
            r = leg(conv, bn, args, kwargs, seed=1000 + rnd)
            rows[name].append(r)
            not_best = ["%.3f" % (r["decile_not_best"][d] / r["decile_plies"][d]) if r["decile_plies"][d] else "-"
                        for d in range(DECILES)]
            lines.append("%-12s games/s %7.2f  steps/s %10.0f  iterations/s %7.1f  finished games %5d  plies per game %6.1f  "
                         "visit share of the move played %.3f  value drops > 0.3 %s\n             move not the most visited, by "
                         "plies 0-9, 10-19, ..., 90+: %s" % (
                             name, r["games_s"], r["steps_s"], r["iter_s"], r["games"], r["plies"] / max(1, r["games"]),
                             r["share"] / max(1, r["plies"]),
                             "%.4f of %d" % (r["value_drops"] / r["value_pairs"], r["value_pairs"]) if r["value_pairs"] else "-",
                             " ".join(not_best)))
            print(lines[-1], flush=True)
    if "off" in rows and rows["off"]:
        for key, what in (("games_s", "finished games/s"), ("steps_s", "MCTS steps/s"), ("iter_s", "iterations/s")):
            off = [r[key] for r in rows["off"]]
            text = "mean %-17s off %10.2f (%.2f .. %.2f)" % (what, statistics.mean(off), min(off), max(off))
            for name, _ in schedules[1:]:
                m = statistics.mean(r[key] for r in rows[name])
                text += "  %s %10.2f (%+.2f %%)" % (name, m, 100.0 * (m / statistics.mean(off) - 1.0))
            lines.append(text)
            print(text)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
