"""What reanalysis costs next to generating ("Reanalysis of stored plies"): positions per second of
training.reanalyse beside the generator's own plies per second at the same visits, what a round spends outside the search, and
the same hand-back of the roots by the route the calls before it allow.

    python tools/reanalyse_rate.py [--network model.npy] [--slots 4096] [--visits 100 400] [--rounds 3]
                                   [--store-seconds 40] [--generator-seconds 20] [--out profiles/reanalyse.txt]

1. The generator CLI plays games at --store-visits for --store-seconds (bf16, --record-values): the stored games.
2. Per visit count V the generator CLI runs for --generator-seconds: its plies per second, from its own "Totals:" line.
3. Per V, training.reanalyse searches --rounds rounds of --slots stored plies with the same net in bf16: positions per second,
   and per round the host clock around read_plies, set_positions, the search, the report and retarget (each call ends in a
   synchronise).
4. One more round at the first V is searched and handed back twice: root_report_device + retarget, and root_report to the host,
   retarget_host per record, the new pairs uploaded.

Without --network the net is 12 blocks x 128 filters of RANDOM weights: rates only, the targets mean nothing."""
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


def generator(network, visits, seconds, path, seed):
    """One run of the generator CLI -> its "Totals:" (plies, seconds, nn_evals, written ...)."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "accelerated_generate_games.py"), "--network", network,
                          "--output-games", path, "--visits", str(visits), "--dtype", "bf16", "--record-values", "--seed",
                          str(seed), "--max-seconds", str(seconds)], cwd=ROOT, capture_output=True, timeout=seconds + 300)
    if res.returncode != 0:
        raise RuntimeError("the generator failed:\n" + res.stderr.decode()[-3000:])
    line = [l for l in res.stdout.decode().splitlines() if l.startswith("Totals: ")][-1]
    return json.loads(line[len("Totals: "):])


def host_route(engine, n):
    """The roots of the first n slots by existing calls: the reports copied to the host, retarget_host per record, the pairs
    uploaded -> (seconds, pairs)."""
    t0 = time.time()
    words = np.zeros((n, link.ROOT_REPORT_WORDS), dtype=np.uint32)
    link.check(link.load().azh_engine_root_report(engine.h, 0, n, words.ctypes.data))
    index, weight, values = [], [], np.zeros(n)
    for i in range(n):
        ix, w, values[i] = link.retarget_host(words[i])
        index.append(ix)
        weight.append(w)
    on_device = (torch.from_numpy(np.concatenate(index).astype(np.int16)).cuda(), torch.from_numpy(np.concatenate(weight)).cuda(),
                 torch.from_numpy(values).cuda())
    torch.cuda.synchronize()
    return time.time() - t0, int(on_device[0].numel())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--network", default=None)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--visits", type=int, nargs="+", default=[100, 400])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--store-visits", type=int, default=16)
    ap.add_argument("--store-seconds", type=int, default=40)
    ap.add_argument("--generator-seconds", type=int, default=20)
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
        say("reanalysis against generation: %s, bf16, %d slots, MI355X" %
            ("12 x 128 RANDOM weights (rates only)" if a.network is None else os.path.basename(a.network), a.slots))
        say("command: python tools/reanalyse_rate.py " + " ".join(sys.argv[1:] if argv is None else argv))
        games = os.path.join(tmp, "games.json")
        totals = generator(network, a.store_visits, a.store_seconds, games, 11)
        say("stored games: the generator CLI at %d visits for %.1f s: %d games written, %d plies played"
            % (a.store_visits, totals["seconds"], totals["written"], totals["plies"]))
        rates = {}
        for v in a.visits:
            t = generator(network, v, a.generator_seconds, os.path.join(tmp, "rate-%d.json" % v), 12)
            rates[v] = t["plies"] / t["seconds"]
            say("generator at %d visits: %d plies in %.1f s = %.0f plies/s (%.0f evals/s)"
                % (v, t["plies"], t["seconds"], rates[v], t["nn_evals"] / t["seconds"]))
        entries = training.load_entries([games])
        arrays = link.entries_to_arrays(entries)
        wanted = a.rounds * a.slots
        spare = (len(a.visits) * wanted + a.slots) * link.MAX_MOVES
        store = link.SampleStore(len(arrays.games), len(arrays.ply_flags), len(arrays.target_index) + spare)
        store.add_arrays(arrays)
        mirror, flags = store.mirror()
        cand, count, _, _ = store.ply_cum()
        c = sum(int(n) for n in count)
        say("the store: %d games, %d plies, %d targets, %d candidate plies" % (len(mirror), len(flags), len(arrays.target_index), c))
        plan = training.reanalyse_plan(mirror, flags, cand, count, store.game_blockers(), 0, len(mirror), min(1.0, wanted / c),
                                       a.slots, seed=1)
        net = link.Net(*model.load_model(network))
        say()
        say("visits  positions  rounds  seconds  positions/s  generator plies/s  | per round, ms: read_plies  set_positions  "
            "search  report  retarget  (after-read and KL)")
        for v in a.visits:
            out = training.reanalyse(store, net, link.DTYPE_BF16, plan, v, a.slots, log=lambda text: None)
            ms = {k: 1e3 * s / out["rounds"] for k, s in out["stage_seconds"].items()}
            say("%6d  %9d  %6d  %7.2f  %11.0f  %17.0f  | %24.2f  %13.2f  %6.1f  %6.2f  %8.2f  %19.1f"
                % (v, out["changed"] + out["unchanged"], out["rounds"], out["seconds"], out["positions_per_second"], rates[v],
                   ms["read_plies"], ms["set_positions"], ms["run"], ms["report"], ms["retarget"], ms["kl"]))
            say("        (%d changed, %d unchanged; mean KL(old || new) %.4f)" % (out["changed"], out["unchanged"], out["mean_kl"]))
        # one round handed back by both routes
        mask, plies = plan[0]
        n = len(plies)
        v = a.visits[0]
        engine = link.Engine(training.reanalysis_config(a.slots, v, mask, int(mirror[:, 1].max()) + 1))
        boards = store.read_plies(plies, targets=False)[0]
        loaded = np.empty((a.slots, 2), dtype=np.uint64)
        loaded[:n, 0] = boards[:, 0] | ((plies[:, 1].astype(np.uint64) & np.uint64(1)) << np.uint64(63))
        loaded[:n, 1] = boards[:, 1]
        loaded[n:] = loaded[0]
        at = np.full(a.slots, plies[0, 1], dtype=np.int32)
        at[:n] = plies[:, 1]
        engine.set_positions(loaded, at)
        engine.run(net, 1 + v, link.DTYPE_BF16)
        engine.sync()
        reports = torch.zeros(a.slots * link.ROOT_REPORT_WORDS, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        host_s, pairs = host_route(engine, n)
        t0 = time.time()
        engine.root_report_device(reports, 0, n)
        t1 = time.time()
        status = store.retarget(plies, reports, mask)
        t2 = time.time()
        say()
        say("one round of %d roots at %d visits handed back (%d new pairs, %d plies changed):" % (n, v, pairs, int(status.sum())))
        say("  on the device: root_report_device %.2f ms + retarget %.2f ms = %.2f ms" % (1e3 * (t1 - t0), 1e3 * (t2 - t1),
                                                                                         1e3 * (t2 - t0)))
        say("  by existing calls: root_report to the host (%.1f MB), retarget_host per record in Python, upload of the pairs: "
            "%.1f ms" % (n * link.ROOT_REPORT_WORDS * 4e-6, 1e3 * host_s))
        say("  (the host route ends with the pairs on the device; no existing call puts them into the store)")
        say()
        say("Not measured: whether training on reanalysed targets makes the loop learn faster.")
        engine.close()
        net.close()
        store.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
