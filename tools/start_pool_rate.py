#!/usr/bin/python
"""What a pool of start positions costs the generator and the surprise pass (profiles/start_pool.txt).

    python tools/start_pool_rate.py --stage generate --path games.json   a fixed time of self-play with a four-map pool in one
                                                                        engine and the same time with one of the maps as the
                                                                        start position: node-evals/s and games/s of each;
                                                                        games.json (pooled, uid order) and games.json.single
                                                                        hold the same number of games
    python tools/start_pool_rate.py --stage surprise --path games.json   the surprise pass over either file: the chunks the
                                                                        pass cuts where the mask changes, and its time
"""
import argparse
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAPS = ["x5o/7/3-3/2-1-2/3-3/7/o5x x",       # the self-play start and its four walls
        "x5o/7/7/7/7/7/o5x x",               # no walls
        "-x4o/2-4/7/2-4/6-/7/o5x x",          # four walls no symmetry keeps
        "x5o/7/2-1-2/7/2-1-2/7/o5x x"]        # four walls every symmetry keeps


def generate(path, seconds, games, visits):
    from ataxxzero_amd import model, selfplay
    conv, bn = model.random_init(2, 128, seed=1)
    kept = {}
    for label, pool in (("four-map pool", MAPS), ("one map (--start-fen)", None)):
        sp = selfplay.SelfPlay(conv, bn, games=games, visits=visits, dtype="bf16", seed=7, streams=1, fen=MAPS[0],
                               start_fens=pool, flags=0)
        sp.set_record_blockers(True)
        sp.set_emit_order(True)
        sp.run(200)
        sp.sync()                                                   # warm-up: code objects, the first games under way
        before, lines = sp.stats(), []
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            sp.run(100)
            lines += sp.drain()
        sp.sync()
        dt = time.perf_counter() - t0
        after = sp.stats()
        print("%s: %d game slots, %d visits, %.1f s: %.0f node-evals/s, %.1f games/s (%d games finished, %d dropped)"
              % (label, games, visits, dt, (after["nn_evals"] - before["nn_evals"]) / dt, (after["games"] - before["games"]) / dt,
                 after["games"] - before["games"], after["dropped"] - before["dropped"]))
        kept[label] = lines
        sp.close()
    n = min(len(v) for v in kept.values())
    for (label, lines), name in zip(kept.items(), (path, path + ".single")):
        with open(name, "wb") as f:
            f.write(b"\n".join(lines[:n]) + b"\n")
        print("%s: %d games written to %s" % (label, n, name))


def surprise(path, dtype):
    import torch  # noqa: F401  (its HIP runtime first: link.require_torch_runtime)
    from ataxxzero_amd import link, model, training
    random.seed(1)
    conv, bn = model.random_init(2, 128, seed=1)
    net = link.Net(conv, bn)
    for name in (path, path + ".single"):
        arrays = link.entries_to_arrays(training.load_entries([name]))
        store = link.SampleStore(len(arrays.games), len(arrays.ply_flags), len(arrays.target_index))
        store.add_arrays(arrays)
        masks = store.game_blockers()
        runs = 1 + int((masks[1:] != masks[:-1]).sum())
        store.surprise(net, link.DTYPES[dtype], 0, 16)                       # warm-up
        for run in range(2):
            t0 = time.perf_counter()
            kl, illegal = store.surprise(net, link.DTYPES[dtype], 0, len(arrays.games))
            dt = time.perf_counter() - t0
            tower, kernel = store.surprise_ms()
            print("surprise pass over %s, %s, run %d: %d games on %d maps, %d plies, %d mask runs (a chunk never spans two), "
                  "%.3f s (tower %.1f ms, kernel %.1f ms by HIP events), %d targets that are no legal moves"
                  % (os.path.basename(name), dtype, run + 1, len(arrays.games), len(set(masks.tolist())), len(kl), runs, dt,
                     tower, kernel, illegal))
        store.close()
    net.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--stage", choices=["generate", "surprise"], required=True)
    ap.add_argument("--path", required=True)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--visits", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    args = ap.parse_args()
    if args.stage == "generate":
        return generate(args.path, args.seconds, args.games, args.visits)
    return surprise(args.path, args.dtype)


if __name__ == "__main__":
    sys.exit(main())
