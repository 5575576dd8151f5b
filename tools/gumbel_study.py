#!/usr/bin/python
"""What the Gumbel root search costs and yields in the generator's own loop (two half-batches, select budget 48, bf16 12x128
tower, steady-state positions loaded as bench.py does), legs one after the other in one process:

    puct400     --visits 400, Dirichlet root, tree reuse, evaluation cache (the default generator)
    cap100      the same with --fast-visits 100 --full-search-fraction 0.25
    fresh16     --visits 16 on a fresh tree every ply without root noise, the mode OFF: the moves are played inside the tower
                launch (the leg the third launch is measured against)
    gumbel16    --visits 16 --gumbel-actions 16: the same search with the root rule and the move-playing launch of its own
    gumbel32    --visits 32 --gumbel-actions 16

Per leg: finished games/s, plies/s (= policy targets/s under Gumbel; under the cap a quarter of them are), search steps/s,
iterations/s.  "third launch" = the difference of the iteration time between gumbel16 and fresh16.

With --target the script also plays --target-games games step by step with the same net through the host (logits and values
from Net.forward) at --visits 16 and reports, over the plies played, the mean total variation distance between the recorded
target and the root's prior: the share of root mass the target moves off the prior.

    python tools/gumbel_study.py [--steps 4] [--target] [--out profiles/gumbel.txt]

Appends its report to --out.  GPU box, repo root."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ataxxzero_amd import link, model, selfplay  # noqa: E402

SNAPSHOT = os.path.join(ROOT, "profiles", "round2_steady_state_positions.npz")

LEGS = {
    "puct400": dict(visits=400, flags=link.FLAG_EVAL_CACHE),
    "cap100": dict(visits=400, flags=link.FLAG_EVAL_CACHE, fast_visits=100, full_fraction=0.25),
    "fresh16": dict(visits=16, flags=link.FLAG_NO_REUSE, dirichlet_weight=0.0),
    "gumbel16": dict(visits=16, gumbel=(16, 50.0, 1.0)),
    "gumbel32": dict(visits=32, gumbel=(16, 50.0, 1.0)),
}


def leg(name, conv, bn, args):
    sp = selfplay.SelfPlay(conv, bn, games=args.games, dtype=args.dtype, seed=1000, streams=2, select_budget=48, **LEGS[name])
    snap = np.load(SNAPSHOT)
    rng = np.random.default_rng(1000)
    n = len(snap["plies"])
    pick = rng.permutation(n) if args.games == n else rng.integers(0, n, size=args.games)
    sp.set_positions(snap["boards"][pick], snap["plies"][pick])
    for _ in range(args.fill // 250):
        sp.run(250)
        sp.drain()
    sp.sync()
    st0 = sp.stats()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sp.run(250)
        sp.fetch()
        sp.drain()
    sp.sync()
    dt = time.perf_counter() - t0
    st = {k: v - st0[k] for k, v in sp.stats().items()}
    sp.close()
    iters = 250 * args.steps
    return {"name": name, "games_s": st["games"] / dt, "plies_s": st["plies"] / dt, "steps_s": st["steps"] / dt,
            "evals_s": st["nn_evals"] / dt, "iter_s": iters / dt, "iter_us": 1e6 * dt / iters}


def target_shift(conv, bn, args):
    """mean and maximum total variation distance between the recorded target and the prior, over the plies of a host-stepped run"""
    net = link.Net(conv, bn, model.BN_EPSILON)
    cfg = selfplay.make_config(args.target_games, 16, seed=77, flags=link.FLAG_NO_REUSE, dirichlet_weight=0.0)
    e = link.Engine(cfg)
    e.set_gumbel(16, 50.0, 1.0)
    v0 = np.full(e.G, 0.5, dtype=np.float32)
    tv = []
    for it in range(args.target_iterations):
        phase = [e.game_state(g).phase for g in range(e.G)]
        e.select()
        need, lb = e.leaves()
        logits, values = net.forward(lb, cfg.blockers, link.DTYPES[args.dtype])
        values = values.reshape(-1)
        for g in range(e.G):
            if phase[g] == 0:
                v0[g] = (np.float32(values[g]) + np.float32(1.0)) * np.float32(0.5)
        e.set_evals(logits.reshape(e.G, -1), values)
        e.backup()
        for g in range(e.G):
            s = e.game_state(g)
            if s.phase == 2 and phase[g] == 1:
                _, info, edges, _ = e.tree(g)
                first, M = int(info[0][0]), int(info[0][1]) & 0xFFFF
                r = np.ascontiguousarray(edges[first:first + M])
                prior, n, W = r[:, 0].copy().view(np.float32), r[:, 1].copy(), r[:, 2].copy().view(np.float32)
                _, counts = link.gumbel_root(prior, W, n, v0[g], link.gumbel_noise(77, s.uid, s.ply, M), 50.0, 1.0)
                target = counts.astype(np.float64) / counts.sum()
                tv.append(0.5 * np.abs(target - prior.astype(np.float64)).sum())
    e.close()
    net.close()
    return tv


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int, default=4, help="timed steps of 250 iterations per leg")
    ap.add_argument("--fill", type=int, default=500, help="untimed iterations after the positions are loaded")
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--target", action="store_true")
    ap.add_argument("--target-games", type=int, default=64)
    ap.add_argument("--target-iterations", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gumbel.txt"))
    args = ap.parse_args()
    selfplay.select_device(0)
    conv, bn = model.random_init(args.blocks, 128, seed=1, perturb_bn=True)
    lines = ["== tools/gumbel_study.py: MEASURED ON THE DEVICE (%s) — %d games in two half-batches, %dx128 %s, randomly "
             "initialised net; %d timed steps of 250 iterations per leg after %d untimed"
             % (link.pci_bus_id(0), args.games, args.blocks, args.dtype, args.steps, args.fill)]
    rows = {}
    for name in args.legs.split(","):
        r = rows[name] = leg(name, conv, bn, args)
        lines.append("%-9s games/s %8.2f  plies/s %9.1f  steps/s %10.0f  evals/s %10.0f  iterations/s %7.1f (%7.1f us each)" % (
            name, r["games_s"], r["plies_s"], r["steps_s"], r["evals_s"], r["iter_s"], r["iter_us"]))
        print(lines[-1], flush=True)
    if "fresh16" in rows and "gumbel16" in rows:
        lines.append("third launch and root rule: gumbel16 - fresh16 = %.1f us per iteration (%.1f %% of fresh16's)" % (
            rows["gumbel16"]["iter_us"] - rows["fresh16"]["iter_us"],
            100.0 * (rows["gumbel16"]["iter_us"] / rows["fresh16"]["iter_us"] - 1.0)))
        print(lines[-1])
    if args.target:
        tv = target_shift(conv, bn, args)
        lines.append("target against prior at --visits 16 --gumbel-actions 16 (%d games stepped through the host, %d plies): total "
                     "variation distance mean %.4f, median %.4f, max %.4f" % (
                         args.target_games, len(tv), float(np.mean(tv)), float(np.median(tv)), float(np.max(tv))))
        print(lines[-1])
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
