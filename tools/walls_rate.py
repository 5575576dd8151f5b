#!/usr/bin/python
"""What the wall masks cost the sample store and what the surprise pass got wrong without them (profiles/walls.txt).

    python tools/walls_rate.py --stage generate --path games.json     the games of tools/device_samples_rate.py (same net, same
                                                                     seeds) written with "blockers"; games.json.nokey: the
                                                                     same lines without the key
    python tools/device_samples_rate.py --stage kernel --path FILE    the gather rates, on either file
    python tools/walls_rate.py --stage surprise --path games.json     the surprise pass over the file, with the masks and with
                                                                     the key stripped (the pass as it ran before): time and KL
"""
import argparse
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def generate(path, games):
    from ataxxzero_amd import model, selfplay
    conv, bn = model.random_init(2, 128, seed=1)
    sp = selfplay.SelfPlay(conv, bn, games=1024, visits=32, dtype="bf16", seed=7)
    sp.set_record_blockers(True)
    lines = []
    while len(lines) < games:
        sp.run(100)
        lines += sp.drain()
    sp.close()
    lines = lines[:games]
    key = b'"blockers":[17,23,25,31],'
    assert all(line[1:1 + len(key)] == key for line in lines)
    with open(path, "wb") as f:
        f.write(b"\n".join(lines) + b"\n")
    with open(path + ".nokey", "wb") as f:
        f.write(b"\n".join(line[:1] + line[1 + len(key):] for line in lines) + b"\n")


def surprise(path, dtype):
    import torch  # noqa: F401  (its HIP runtime first: link.require_torch_runtime)
    from ataxxzero_amd import link, model, training
    random.seed(1)
    entries = training.load_entries([path])
    conv, bn = model.random_init(2, 128, seed=1)
    net = link.Net(conv, bn)
    for label, games in (("with the games' masks", entries),
                         ("key stripped (no mask)", [{k: v for k, v in e.items() if k != "blockers"} for e in entries])):
        arrays = link.entries_to_arrays(games)
        store = link.SampleStore(len(arrays.games), len(arrays.ply_flags), len(arrays.target_index))
        store.add_arrays(arrays)
        masks = store.game_blockers()
        store.surprise(net, link.DTYPES[dtype], 0, 16)                       # warm-up: code objects, the tower's buffers
        for run in range(2):
            t0 = time.perf_counter()
            kl, illegal = store.surprise(net, link.DTYPES[dtype], 0, len(arrays.games))
            seconds = time.perf_counter() - t0
            tower, kernel = store.surprise_ms()
            k = kl[(store.mirror()[1] & (link.SAMPLES_PLY_PASS | link.SAMPLES_PLY_BAD)) == 0].astype(np.float64)
            print("surprise pass, %s, %s, run %d: %d games (%d with walls), %d plies in %.3f s (tower %.1f ms, kernel %.1f ms "
                  "by HIP events); KL mean %.4f, median %.4f, max %.4f; %d targets that are no legal moves"
                  % (label, dtype, run + 1, len(arrays.games), int((masks != 0).sum()), len(kl), seconds, tower, kernel,
                     k.mean(), float(np.median(k)), k.max(), illegal))
        store.close()
    net.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--stage", choices=["generate", "surprise"], required=True)
    ap.add_argument("--path", required=True)
    ap.add_argument("--games", type=int, default=2000)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    args = ap.parse_args()
    if args.stage == "generate":
        return generate(args.path, args.games)
    return surprise(args.path, args.dtype)


if __name__ == "__main__":
    sys.exit(main())
