#!/usr/bin/python
"""train.py with and without device-resident samples, and the gather kernel by itself, on one GPU (run from the repo root):

    python tools/device_samples_rate.py [--games 2000] [--steps 1000]

Self-play games of a random 2-block net are written to a temporary file; `train.py --steps N` is timed on it three times —
without flags (the host pipeline), with --device-samples and with --device-draws — each in a process of its own, wall time
from start to exit; then one process times SampleStore.add_entries and, by HIP events on torch's stream, the gather at
minibatch sizes 512 and 2048 (and 32768, where the device and not the host's enqueue rate sets the time) with host draws
(check of the draws and staging copy included) and with device draws.  --aux: the games carry "blockers" (the walls of the
self-play start: a game's owners are found from its line alone), the store also holds the games' owners, and the kernels that
write the auxiliary targets as well (ownership, score, reply, weights: 4 * 885 more bytes per sample) are timed beside the
others."""
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
SAMPLE_BYTES = 4 * (196 + 833 + 1)
AUX_BYTES = 4 * (49 + 1 + 833 + 2)


def generate(path, games, record_blockers=False):
    from ataxxzero_amd import model, selfplay
    conv, bn = model.random_init(2, 128, seed=1)
    sp = selfplay.SelfPlay(conv, bn, games=1024, visits=32, dtype="bf16", seed=7)
    if record_blockers:                  # the owners are found from a line alone: it has to name the walls of its board
        sp.set_record_blockers(True)
    lines = []
    while len(lines) < games:
        sp.run(100)
        lines += sp.drain()
    sp.close()
    with open(path, "w") as f:
        f.write(b"\n".join(lines[:games]).decode() + "\n")


def kernel_times(path, aux=False):
    import torch
    from ataxxzero_amd import link, training
    random.seed(1)
    entries = training.load_entries([path])
    t0 = time.perf_counter()
    arrays = link.entries_to_arrays(entries, aux=aux)
    t1 = time.perf_counter()
    store = link.SampleStore(len(arrays.games), len(arrays.ply_flags), len(arrays.target_index))
    store.add_arrays(arrays)
    t2 = time.perf_counter()
    c = store.counts()
    print("store: %(games)d games, %(plies)d plies, %(targets)d targets, %(bad_plies)d bad plies" % c)
    print("add_entries: %.2f s converting the parsed lines on the host (training._entry_arrays per entry), %.3f s checking "
          "and copying them to the device" % (t1 - t0, t2 - t1))
    if aux:
        print("owners: %d of %d games have them" % (int(store.game_owners().any(axis=1).sum()), c["games"]))
    for n in (512, 2048, 32768):     # (32768: large enough for the device, not the host's enqueue rate, to set the time)
        out, aux_out = store.outputs(n), store.aux_outputs(n) if aux else None
        draws = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        store.draw_gather(n, 1, 0, 0, c["games"], 0.0, out=out, draws_out=draws)
        host_draws = draws.cpu().numpy()[:, :3].copy()
        assert (host_draws >= 0).all()
        calls = [("host draws", SAMPLE_BYTES, lambda k: store.gather(host_draws, 0.0, out=out)),
                 ("device draws", SAMPLE_BYTES, lambda k: store.draw_gather(n, 1, k, 0, c["games"], 0.0, out=out))]
        if aux:
            calls += [("host draws, aux", SAMPLE_BYTES + AUX_BYTES,
                       lambda k: store.gather(host_draws, 0.0, out=aux_out, aux=True)),
                      ("device draws, aux", SAMPLE_BYTES + AUX_BYTES,
                       lambda k: store.draw_gather(n, 1, k, 0, c["games"], 0.0, out=aux_out, aux=True))]
        for name, sample_bytes, call in calls:
            for k in range(5):
                call(k)
            torch.cuda.synchronize()
            reps = 200
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            start.record()
            for k in range(reps):
                call(k)
            stop.record()
            w1 = time.perf_counter()
            torch.cuda.synchronize()
            us = start.elapsed_time(stop) * 1000.0 / reps
            print("gather, %4d samples, %s: %7.1f us per minibatch by HIP events (%.1f us of host time per call to "
                  "enqueue), %.1f GB/s written" % (n, name.ljust(17 if aux else 12), us, (w1 - w0) * 1e6 / reps,
                                                   n * sample_bytes / us / 1e3))
    assert store.status() == 0
    store.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--games", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--aux", action="store_true", help="also time the kernels that write the auxiliary targets")
    ap.add_argument("--stage", choices=["generate", "kernel"], help=argparse.SUPPRESS)
    ap.add_argument("--path", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.stage == "generate":
        return generate(args.path, args.games, args.aux)
    if args.stage == "kernel":
        return kernel_times(args.path, args.aux)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "games.json")
        me = [sys.executable, os.path.abspath(__file__)]
        subprocess.run(me + ["--stage", "generate", "--path", path, "--games", str(args.games)] + (["--aux"] if args.aux else []),
                       check=True, cwd=ROOT, timeout=600)
        with open(path) as f:
            plies = [len(json.loads(line)["moves"]) for line in f]
        print("%d self-play games (random 2x128 net, 32 visits), %d plies" % (len(plies), sum(plies)))
        for flags in ([], ["--device-samples"], ["--device-draws"]):
            t0 = time.perf_counter()
            res = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--games", path, "--new-path",
                                  os.path.join(tmp, "model.npy"), "--steps", str(args.steps)] + flags, cwd=ROOT,
                                 capture_output=True, timeout=900)
            wall = time.perf_counter() - t0
            if res.returncode != 0:
                print(res.stderr.decode()[-2000:])
                return 1
            last = [l for l in res.stdout.decode().splitlines() if l.startswith("Step:")][-1]
            print("train.py --steps %d %-17s: %6.1f s wall   (last log line: %s)" % (args.steps, " ".join(flags) or "(host pipeline)",
                                                                                   wall, last.strip()))
            sys.stdout.flush()
        subprocess.run(me + ["--stage", "kernel", "--path", path] + (["--aux"] if args.aux else []), check=True, cwd=ROOT,
                       timeout=600)
    return 0


if __name__ == "__main__":
    sys.exit(main())
