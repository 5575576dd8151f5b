"""What the lambda-returns pass costs and how far its targets lie from the game's result ("Lambda-returns as value
targets"): seconds of SampleStore.value_returns over a games file beside SampleStore.prove on the same store in the same run,
and the distribution of |G_p - z_p| at lambda 0.5 and 0.9, without and with the proofs of a depth-3 pass.

    python tools/value_lambda_rate.py [--network model.npy] [--store-seconds 12] [--max-plies 200000] [--repeats 5]
                                      [--out profiles/value_lambda.txt]

1. The generator CLI plays games at 16 visits with --record-values for --store-seconds (bf16): the games file; its first games
   up to --max-plies plies go into one store.
2. value_returns over every game, --repeats times per lambda, each timed by the host clock (the call returns after
   completion; the first call of the store also allocates the array and fills it).  A sample of games is compared with
   link.value_returns_host bit for bit.
3. |G_p - z_p| over every stored ply, read back with read_value_returns.
4. prove(depth 3) over every game, timed the same way, then step 2 and 3 again: the returns now start from the proofs.

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

EDGES = (0.0, 0.01, 0.1, 0.25, 0.5, 1.0, 1.5, 2.0)


def generate(network, seconds, path):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "accelerated_generate_games.py"), "--network", network,
                          "--output-games", path, "--visits", "16", "--dtype", "bf16", "--record-values", "--seed", "11",
                          "--max-seconds", str(seconds)], cwd=ROOT, capture_output=True, timeout=seconds + 300)
    if res.returncode != 0:
        raise RuntimeError("the generator failed:\n" + res.stderr.decode()[-3000:])
    line = [l for l in res.stdout.decode().splitlines() if l.startswith("Totals: ")][-1]
    return json.loads(line[len("Totals: "):])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--network", default=None)
    ap.add_argument("--store-seconds", type=int, default=12)
    ap.add_argument("--max-plies", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=5)
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
        say("lambda-returns over stored plies: games of %s, MI355X" %
            ("12 x 128 RANDOM weights" if a.network is None else os.path.basename(a.network)))
        say("command: python tools/value_lambda_rate.py " + " ".join(sys.argv[1:] if argv is None else argv))
        games = os.path.join(tmp, "games.json")
        totals = generate(network, a.store_seconds, games)
        entries = training.load_entries([games])
        kept, plies = [], 0
        for e in entries:
            if plies + len(e["boards"]) > a.max_plies:
                break
            kept.append(e)
            plies += len(e["boards"])
        lengths = np.array([len(e["boards"]) for e in kept])
        say("games file: the generator CLI at 16 visits with --record-values for %.1f s: %d games written; the first %d games, "
            "%d plies, are stored (plies per game: mean %.1f, median %d, max %d); %d of them carry values"
            % (totals["seconds"], totals["written"], len(kept), plies, lengths.mean(), int(np.median(lengths)), lengths.max(),
               sum("values" in e for e in kept)))
        arrays = link.entries_to_arrays(kept)
        store = link.SampleStore(len(arrays.games), len(arrays.ply_flags), len(arrays.target_index))
        store.add_arrays(arrays)
        mirror, _ = store.mirror()
        G = len(mirror)
        pairs = np.array([(g, p) for g in range(G) for p in range(int(mirror[g][1]))], dtype=np.int32)
        z = np.array([1.0 if (int(mirror[g][2]) & 0xFF) == 1 + (p & 1) else -1.0 for g, p in pairs.tolist()])
        first = np.concatenate([[0], np.cumsum(lengths)])

        def passes(proofs, label):
            say()
            say("value_returns over %d games, %d plies, %s: host-clock seconds per call" % (G, plies, label))
            for lam in (0.5, 0.9):
                seconds = []
                for _ in range(a.repeats):
                    t0 = time.time()
                    store.value_returns(0, G, lam)
                    seconds.append(time.time() - t0)
                got, present = store.read_value_returns(pairs)
                assert present.all()
                for g in range(0, G, max(G // 64, 1)):                       # a sample of games against the host function
                    lo, hi = int(first[g]), int(first[g + 1])
                    want = link.value_returns_host(arrays.values[lo:hi], None if proofs is None else proofs[lo:hi],
                                                   int(mirror[g][2]) & 0xFF, lam)
                    assert got[lo:hi].tobytes() == want.tobytes(), (g, lam)
                d = np.abs(got - z)
                hist = np.histogram(d, bins=EDGES)[0]
                say("  lambda %.1f: %s  -> best %.6f s, %.3e plies/s" % (lam, "  ".join("%.6f" % s for s in seconds), min(seconds),
                                                                          plies / min(seconds)))
                say("    |G_p - z_p|: mean %.4f, median %.4f, 90th percentile %.4f, max %.4f; share with the sign of z: %.3f"
                    % (d.mean(), np.median(d), np.percentile(d, 90), d.max(), float(((got > 0) == (z > 0)).mean())))
                bins = ["[%g,%g%s" % (lo, hi, "]" if hi == EDGES[-1] else ")") for lo, hi in zip(EDGES[:-1], EDGES[1:])]
                say("    plies per bin %s: %s" % (" ".join(bins), " ".join(str(int(h)) for h in hist)))

        store.prove(0, 1, 1)                                                 # the first launch of the process is not timed
        store.close()
        store = link.SampleStore(len(arrays.games), len(arrays.ply_flags), len(arrays.target_index))
        store.add_arrays(arrays)
        passes(None, "no proofs (the first call allocates and fills the array)")
        t0 = time.time()
        s = store.prove(0, G, 3)
        seconds = time.time() - t0
        say()
        say("prove(depth 3, no node limit) over the same store: %.6f s; %d plies searched, %d proven (%d wins, %d losses), %d "
            "contradict their game's result" % (seconds, s["visited"], s["wins"] + s["losses"], s["wins"], s["losses"],
                                                s["contradicted"]))
        passes(store.proofs(pairs)[0], "after the proof pass")
        store.close()
        say()
        say("Not measured: whether training on lambda-returns makes the loop learn faster.")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
