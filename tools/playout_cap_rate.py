#!/usr/bin/python
"""What playout cap randomization buys the generator: its own loop (two half-batches, evaluation cache, select budget 48,
bf16 12x128 tower, steady-state positions loaded as bench.py does) with the cap off against the cap on, legs alternating
in one process.  Per leg: plies/s, finished games/s, FULL plies/s (plies/s x the share of FULL plies among the plies the
leg's finished records carry) and how much longer the tower launch — which carries the move-playing workgroups — lasts
than the bare tower at the leg's mean batch: with the moves inside the tower launch there is no per-iteration
observable of "the workers outlasted the tiles", so the mean excess per launch stands in for that share.

    python tools/playout_cap_rate.py [--pairs 3] [--steps 8] [--out profiles/playout_cap.txt]

With --forced-playouts K the two legs are forced playouts and policy target pruning off against on (k = K) instead — the cap
off in both, or on in both with --cap — and the report adds the mean share of a ply's visits the pruning took out of its
record, over the plies the mode acts on:

    python tools/playout_cap_rate.py --forced-playouts 2 [--cap] --out profiles/forced_playouts.txt

With --random-symmetry the two legs are the random symmetry per evaluation off against on (the cap and forced playouts as
given, the same in both legs):

    python tools/playout_cap_rate.py --random-symmetry --out profiles/random_symmetry.txt

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


def staged_plies(words):
    """(kind word, word 5, the ply's target words) of every ply of the staged record words (layout: link.records), dropped
    games' markers skipped; a word that is not a header is stepped over until the next magic"""
    pos = 0
    while pos + link.REC_HDR_WORDS <= len(words):
        if words[pos] != link.RECORD_MAGIC:
            pos += 1
            continue
        n, q, kind = int(words[pos + link.REC_WORDS]), pos + link.REC_HDR_WORDS, int(words[pos + link.REC_KIND])
        if kind & link.REC_KIND_MASK != link.REC_KIND_DROPPED:
            for _ in range(int(words[pos + link.REC_PLIES])):
                nd = int(words[q + 4]) >> 16
                yield kind, int(words[q + 5]), words[q + link.REC_PLY_WORDS:q + link.REC_PLY_WORDS + nd]
                q += link.REC_PLY_WORDS + nd
        pos += max(n, link.REC_HDR_WORDS)


def pruned_share(words, visits):
    """(sum over the acting plies of 1 - written visits / `visits`, acting plies) over the staged record words of an engine
    with forced playouts on: the plies of games that carry the mode's bit, FULL ones if the cap is on"""
    share, acting = 0.0, 0
    for kind, word5, targets in staged_plies(words):
        if kind & link.REC_KIND_FORCED and (word5 or not kind & link.REC_KIND_PLAYOUT_CAP):
            share += 1.0 - min(1.0, float((targets >> 16).sum()) / visits)
            acting += 1
    return share, acting


def full_share(words):
    """(FULL plies, plies) over the staged record words"""
    full = [word5 for _, word5, _ in staged_plies(words)]
    return sum(full), len(full)


def leg(conv, bn, args, cap, seed, forced=0.0, symmetry=False):
    sp = selfplay.SelfPlay(conv, bn, games=args.games, visits=args.visits, dtype=args.dtype, seed=seed, streams=2,
                           flags=link.FLAG_EVAL_CACHE, select_budget=48,
                           fast_visits=args.fast_visits if cap else 0, full_fraction=args.full_search_fraction,
                           forced_playouts=forced, random_symmetry=symmetry)
    snap = np.load(SNAPSHOT)
    rng = np.random.default_rng(seed)
    pick = rng.permutation(len(snap["plies"])) if args.games == len(snap["plies"]) else rng.integers(0, len(snap["plies"]), size=args.games)
    sp.set_positions(snap["boards"][pick], snap["plies"][pick])
    for _ in range(args.fill // 250):
        sp.run(250)
        sp.drain()
    sp.sync()
    st0 = sp.stats()
    sp.timing_reset(16)
    full = plies = acting = 0
    pruned = 0.0
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sp.run(250)
        sp.fetch()
        for e in sp.engines:
            f, p = full_share(e.staged_records())
            full, plies = full + f, plies + p
            if forced:
                s, a = pruned_share(e.staged_records(), args.visits)
                pruned, acting = pruned + s, acting + a
        sp.drain()
    sp.sync()
    dt = time.perf_counter() - t0
    st = {k: v - st0[k] for k, v in sp.stats().items()}
    tm = sp.timing()
    iters = 250 * args.steps
    batch = st["nn_evals"] / (2.0 * iters)                      # mean leaves per tower launch (two half-batches)
    tower_ms = tm["net_ms"] / max(1, tm["iterations"])
    bare_ms = sp.net.bench(max(1, int(round(batch))), 20, link.DTYPES[args.dtype])
    sp.close()
    share = 1.0 if not cap else (full / plies if plies else float("nan"))   # (cap off: every ply is searched in full)
    return {"symmetry": symmetry, "forced": forced, "pruned_share": pruned / acting if acting else float("nan"), "cap": cap, "plies_s": st["plies"] / dt, "games_s": st["games"] / dt,
            "full_share": share, "full_plies_s": st["plies"] / dt * share, "evals_s": st["nn_evals"] / dt,
            "plies_per_iter": st["plies"] / (2.0 * iters), "batch": batch, "tower_us": 1e3 * tower_ms,
            "bare_us": 1e3 * bare_ms, "iter_s": iters / dt}


def row(r):
    return ("%-4s plies/s %8.1f  games/s %6.2f  full plies/s %8.1f (share %.3f)  evals/s %9.0f  iterations/s %7.1f  "
            "moves due per launch %5.1f  leaves per launch %6.0f  tower launch %6.1f us, bare tower at that batch %6.1f us (excess %5.1f us)" % (
                ("sym" if r["symmetry"] else "none") if r.get("by_symmetry") else
                ("k=%g" % r["forced"] if r["forced"] else "k=0") if r["by_forced"] else "on" if r["cap"] else "off", r["plies_s"], r["games_s"], r["full_plies_s"], r["full_share"],
                r["evals_s"], r["iter_s"], r["plies_per_iter"], r["batch"], r["tower_us"], r["bare_us"], r["tower_us"] - r["bare_us"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--visits", type=int, default=400)
    ap.add_argument("--fast-visits", type=int, default=100)
    ap.add_argument("--full-search-fraction", type=float, default=0.25)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8, help="timed steps of 250 iterations per leg")
    ap.add_argument("--fill", type=int, default=1000, help="untimed iterations after the positions are loaded")
    ap.add_argument("--forced-playouts", type=float, default=0.0, metavar="K",
                    help="the legs are forced playouts off against on (k = K) instead of the cap off against on")
    ap.add_argument("--cap", action="store_true", help="with --forced-playouts: the playout cap on in both legs")
    ap.add_argument("--random-symmetry", action="store_true",
                    help="the legs are the random symmetry per evaluation off against on (cap with --cap, forced playouts with "
                         "--forced-playouts K, the same in both legs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "playout_cap.txt"))
    args = ap.parse_args()
    selfplay.select_device(0)
    conv, bn = model.random_init(args.blocks, 128, seed=1, perturb_bn=True)
    lines = ["== tools/playout_cap_rate.py: MEASURED ON THE DEVICE (%s) — %d games in two half-batches, %dx128 %s, visits %d; "
             "cap on = --fast-visits %d --full-search-fraction %.2f; %d timed steps of 250 iterations per leg after %d untimed"
             % (link.pci_bus_id(0), args.games, args.blocks, args.dtype, args.visits, args.fast_visits,
                args.full_search_fraction, args.steps, args.fill)]
    rows = []
    by_symmetry = args.random_symmetry
    by_forced = args.forced_playouts > 0 and not by_symmetry
    if by_symmetry:
        lines[0] += "; legs: random symmetry per evaluation off against on, the cap %s and forced playouts k = %g in both" % (
            "on" if args.cap else "off", args.forced_playouts)
    if by_forced:
        lines[0] += "; legs: forced playouts off against k = %g, the cap %s in both" % (args.forced_playouts, "on" if args.cap else "off")
    for pair in range(args.pairs):
        for second in (False, True):
            if by_symmetry:
                r = leg(conv, bn, args, args.cap, seed=1000 + pair, forced=args.forced_playouts, symmetry=second)
            elif by_forced:
                r = leg(conv, bn, args, args.cap, seed=1000 + pair, forced=args.forced_playouts if second else 0.0)
            else:
                r = leg(conv, bn, args, second, seed=1000 + pair)
            r["by_forced"], r["by_symmetry"], r["second"] = by_forced, by_symmetry, second
            rows.append(r)
            lines.append(row(r) + ("  visits pruned per acting ply %.4f" % r["pruned_share"] if r["forced"] else ""))
            print(lines[-1], flush=True)
    for key, name in (("plies_s", "plies/s"), ("games_s", "finished games/s"), ("full_plies_s", "full plies/s")):
        off = [r[key] for r in rows if not r["second"]]
        on = [r[key] for r in rows if r["second"]]
        m_off, m_on = statistics.mean(off), statistics.mean(on)
        lines.append("mean %-17s off %9.2f  on %9.2f  ratio %s" % (name, m_off, m_on, "%.3f" % (m_on / m_off) if m_off else "-"))
        print(lines[-1])
    if by_forced:
        lines.append("mean share of a ply's visits pruned from its record, over the plies the mode acts on: %.4f"
                     % statistics.mean(r["pruned_share"] for r in rows if r["second"]))
    bound = args.visits / (args.full_search_fraction * args.visits + (1 - args.full_search_fraction) * args.fast_visits)
    for key, name in (("iter_s", "iterations/s"), ("evals_s", "evaluations/s")) if by_symmetry else ():
        off = [r[key] for r in rows if not r["second"]]
        on = [r[key] for r in rows if r["second"]]
        lines.append("mean %-17s off %9.2f  on %9.2f  ratio %.3f  (off legs' own spread: %.2f .. %.2f)" % (
            name, statistics.mean(off), statistics.mean(on), statistics.mean(on) / statistics.mean(off), min(off), max(off)))
        print(lines[-1])
    if not by_forced and not by_symmetry:
        lines.append("(visits / mean threshold = %.2fx: arithmetic, not a measurement, and no bound — a re-rooted root inherits visits, "
                     "and one that already meets the fast threshold plays after its root evaluation alone)" % bound)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
