#!/usr/bin/python
"""Policy surprise weighting on one GPU (run from the repo root): the surprise pass over a games file, split into tower and
surprise kernel by HIP events; the KL distribution for a random net and for a net trained on those games; train.py with and
without --surprise-weight.

    python tools/surprise_weighting_rate.py [--games 2000] [--steps 1000]

The games are those of tools/device_samples_rate.py (self-play of a random 2x128 net at 32 visits, written to a temporary file).
`train.py --steps N --old-path random-12x128.npy` is timed with --device-draws and with --surprise-weight 0.5, twice in turn, each
in a process of its own, wall time from start to exit; the net the first run writes is the "trained" one of the KL table."""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def surprise_stage(path, nets):
    import numpy as np
    from ataxxzero_amd import link, model, training
    random.seed(1)
    entries = training.load_entries([path])
    arrays = link.entries_to_arrays(entries)
    store = link.SampleStore(len(arrays.games), len(arrays.ply_flags), len(arrays.target_index))
    store.add_arrays(arrays)
    c = store.counts()
    print("store: %(games)d games, %(plies)d plies, %(targets)d targets, %(bad_plies)d bad plies" % c)
    flags = store.mirror()[1]
    sample = (flags & (link.SAMPLES_PLY_PASS | link.SAMPLES_PLY_BAD)) == 0
    for name, net_path in nets:
        net = link.Net(*model.load_model(net_path))
        for dtype in ("bf16", "f32"):
            for run in range(3):            # (the first run of a dtype also packs the net's weights for it)
                t0 = time.perf_counter()
                kl, illegal = store.surprise(net, link.DTYPES[dtype], 0, c["games"])
                wall = time.perf_counter() - t0
                tower, kernel = store.surprise_ms()
                print("surprise pass, %-7s net, %-4s, run %d: %7.1f ms wall; by HIP events %7.1f ms board packing + tower, "
                      "%6.2f ms surprise kernel (%d chunks)" % (name, dtype, run, wall * 1e3, tower, kernel,
                                                                 -(-c["plies"] // 16384)))
            k = kl[sample].astype(np.float64)
            print("KL(target || prior), %-7s net, %-4s: %d plies; mean %.4f, median %.4f, p90 %.4f, p99 %.4f, max %.4f; %d exactly 0;"
                  " %d targets that are no legal moves" % (name, dtype, len(k), k.mean(), np.median(k), np.percentile(k, 90),
                                                           np.percentile(k, 99), k.max(), int((k == 0).sum()), illegal))
        net.close()
    store.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--games", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--stage", choices=["generate", "surprise", "old"], help=argparse.SUPPRESS)
    ap.add_argument("--path", help=argparse.SUPPRESS)
    ap.add_argument("--nets", nargs="*", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.stage == "generate":
        import device_samples_rate
        return device_samples_rate.generate(args.path, args.games)
    if args.stage == "old":
        from ataxxzero_amd import model
        return model.save_model(args.path, *model.random_init(12, 128, seed=5))
    if args.stage == "surprise":
        return surprise_stage(args.path, [tuple(n.split("=", 1)) for n in args.nets])
    with tempfile.TemporaryDirectory() as tmp:
        path, old = os.path.join(tmp, "games.json"), os.path.join(tmp, "old.npy")
        me = [sys.executable, os.path.abspath(__file__)]
        subprocess.run(me + ["--stage", "generate", "--path", path, "--games", str(args.games)], check=True, cwd=ROOT, timeout=600)
        subprocess.run(me + ["--stage", "old", "--path", old], check=True, cwd=ROOT, timeout=600)
        with open(path) as f:
            plies = [len(json.loads(line)["moves"]) for line in f]
        print("%d self-play games (random 2x128 net, 32 visits), %d plies" % (len(plies), sum(plies)))
        news = []
        # (twice in turn: the first run of a process order also pays the first use of the convolution kernels' caches)
        for flags in (["--device-draws"], ["--surprise-weight", "0.5"]) * 2:
            news.append(os.path.join(tmp, "new%d.npy" % len(news)))
            t0 = time.perf_counter()
            res = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--games", path, "--old-path", old,
                                  "--new-path", news[-1], "--steps", str(args.steps)] + flags, cwd=ROOT, capture_output=True,
                                 timeout=900)
            wall = time.perf_counter() - t0
            if res.returncode != 0:
                print(res.stderr.decode()[-2000:])
                return 1
            lines = res.stdout.decode().splitlines()
            last = [l for l in lines if l.startswith("Step:")][-1]
            print("train.py --steps %d %-22s: %6.1f s wall   (last log line: %s)" % (args.steps, " ".join(flags), wall, last.strip()))
            for l in lines:
                if l.startswith("Policy surprise:"):
                    print("    " + l)
            sys.stdout.flush()
        subprocess.run(me + ["--stage", "surprise", "--path", path, "--nets", "random=" + old, "trained=" + news[0]], check=True,
                       cwd=ROOT, timeout=600)
    return 0


if __name__ == "__main__":
    sys.exit(main())
