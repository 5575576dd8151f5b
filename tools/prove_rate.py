"""What the proof pass costs and finds ("Proven outcomes for stored plies"): plies and nodes per second of
SampleStore.prove over a games file beside azh_alphabeta_search on the same positions, the share of plies proven and of proofs
that contradict the game's result per depth, and train.py's wall time with and without the flag.

    python tools/prove_rate.py [--network model.npy] [--store-seconds 12] [--max-plies 200000] [--budget 4096]
                               [--train-steps 1000] [--out profiles/prove.txt]

1. The generator CLI plays games at 16 visits for --store-seconds (bf16, --record-blockers): the games file; its first games
   up to --max-plies plies go into a store per measurement.
2. Per (depth, budget) in (2, 0), (3, 0), (5, B), (8, B): one prove() over every game of a fresh store, timed by the host clock
   (the call returns after completion); then link.alphabeta_search of the same positions read back with read_plies, timed the same
   way (that call allocates, copies the boards in and the answers out).
3. train.py --steps N --device-samples on the file, then the same with --prove-depth 3 --prove-policy: wall seconds, and the
   trainer's own "Proofs:" line.

Without --network the net is 12 blocks x 128 filters of RANDOM weights: its games are what a first generation's look like."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch  # noqa: F401  (before the library is loaded: link.require_torch_runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ataxxzero_amd import link, model, training  # noqa: E402


def generate(network, seconds, path):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "accelerated_generate_games.py"), "--network", network,
                          "--output-games", path, "--visits", "16", "--dtype", "bf16", "--record-blockers", "--seed", "11",
                          "--max-seconds", str(seconds)], cwd=ROOT, capture_output=True, timeout=seconds + 300)
    if res.returncode != 0:
        raise RuntimeError("the generator failed:\n" + res.stderr.decode()[-3000:])
    line = [l for l in res.stdout.decode().splitlines() if l.startswith("Totals: ")][-1]
    return json.loads(line[len("Totals: "):])


def trainer(games, steps, extra):
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.time()
        res = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--steps", str(steps), "--games", games,
                              "--new-path", os.path.join(tmp, "new.npy"), "--device-samples"] + extra, cwd=ROOT,
                             capture_output=True, timeout=1200)
        seconds = time.time() - t0
    if res.returncode != 0:
        raise RuntimeError("train.py failed:\n" + res.stderr.decode()[-3000:])
    return seconds, [l for l in res.stdout.decode().splitlines() if l.startswith("Proofs:")]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--network", default=None)
    ap.add_argument("--store-seconds", type=int, default=12)
    ap.add_argument("--max-plies", type=int, default=200000)
    ap.add_argument("--budget", type=int, default=4096)
    ap.add_argument("--train-steps", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as tmp:
        network = a.network
        if network is None:
            network = os.path.join(tmp, "random-12x128.npy")
            model.save_model(network, *model.random_init(12, 128, seed=1))
        say("proof pass over stored plies: games of %s, MI355X" %
            ("12 x 128 RANDOM weights" if a.network is None else os.path.basename(a.network)))
        say("command: python tools/prove_rate.py " + " ".join(sys.argv[1:] if argv is None else argv))
        games = os.path.join(tmp, "games.json")
        totals = generate(network, a.store_seconds, games)
        entries = training.load_entries([games])
        kept, plies = [], 0
        for e in entries:
            if plies + len(e["boards"]) > a.max_plies:
                break
            kept.append(e)
            plies += len(e["boards"])
        say("games file: the generator CLI at 16 visits for %.1f s: %d games written; the first %d games, %d plies, are stored"
            % (totals["seconds"], totals["written"], len(kept), plies))
        arrays = link.entries_to_arrays(kept)
        say()
        say("depth  budget  plies searched  seconds  plies/s      nodes  nodes/s   | proven  share   wins  losses  contradicted  "
            "share of proven | alphabeta_search: seconds  nodes/s")
        for depth, budget in ((2, 0), (3, 0), (5, a.budget), (8, a.budget)):
            store = link.SampleStore(len(arrays.games), len(arrays.ply_flags), len(arrays.target_index))
            store.add_arrays(arrays)
            mirror, _ = store.mirror()
            if depth == 2:
                store.prove(0, 1, 1)                               # the first launch of the process is not timed
                store.close()
                store = link.SampleStore(len(arrays.games), len(arrays.ply_flags), len(arrays.target_index))
                store.add_arrays(arrays)
            t0 = time.time()
            s = store.prove(0, len(mirror), depth, budget)
            seconds = time.time() - t0
            pairs = np.array([(g, p) for g in range(len(mirror)) for p in range(int(mirror[g][1]))], dtype=np.int32)
            boards = store.read_plies(pairs, targets=False)[0].copy()
            boards[:, 0] |= (pairs[:, 1].astype(np.uint64) & np.uint64(1)) << np.uint64(63)
            walls = store.game_blockers()[pairs[:, 0]]
            t0 = time.time()
            found = link.alphabeta_search(boards, walls, depth, budget, outputs=("values", "nodes"))
            plain = time.time() - t0
            proven = s["wins"] + s["losses"]
            assert int(found.nodes.sum()) == s["nodes"] or s["visited"] != len(pairs)
            say("%5d  %6d  %14d  %7.3f  %7.0f  %9.3e  %7.2e   | %6d  %5.3f  %5d  %6d  %12d  %15.3f | %25.3f  %7.2e"
                % (depth, budget, s["visited"], seconds, s["visited"] / seconds, s["nodes"], s["nodes"] / seconds, proven,
                   proven / max(s["visited"], 1), s["wins"], s["losses"], s["contradicted"], s["contradicted"] / max(proven, 1),
                   plain, int(found.nodes.sum()) / plain))
            store.close()
        say()
        kept_path = os.path.join(tmp, "kept.json")
        with open(kept_path, "w") as f:
            for e in kept:
                f.write(json.dumps(e) + "\n")
        for extra in ([], ["--prove-depth", "3", "--prove-policy"], []):
            seconds, proofs = trainer(kept_path, a.train_steps, extra)
            say("train.py --steps %d --device-samples %s: %.1f s wall%s" % (a.train_steps, " ".join(extra), seconds,
                                                                            "".join("\n    " + p for p in proofs)))
        say()
        say("Not measured: whether training on proven outcomes makes the loop learn faster.")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
