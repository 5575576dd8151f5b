"""Visits per second of the single-position search (uai.Searcher) with K leaves per iteration.

For K in --ks: a `go movetime` search (--movetime-ms) of a 12x128 net (random weights: the rate does not depend on them)
in f16 on the start position and three mid-game positions, each K in its own engine as uai.Searcher builds it.  Reported:
root visits per second, iterations, the HIP-event time per iteration of the tree launch and of the tower launch (every
iteration sampled), and collisions per path.  K = 1 is the one-leaf search exactly as uai.Searcher runs it.

    python tools/uai_nps.py [--movetime-ms 1000] [--ks 1,8,16,32,48,64] [--out profiles/FILE.txt]
"""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ataxxzero_amd import link, model, uai  # noqa: E402

POSITIONS = [
    ("start", "x5o/7/7/7/7/7/o5x x"),
    ("mid-1", "xxx1ooo/xx3oo/x2o2x/3x3/o2x2o/oo3xx/ooo1xxx x"),
    ("mid-2", "2xxoo2/1xxxooo/xxo1oxx/ooxxxoo/1oxoo2/2oxx3/3o3 o"),
    ("mid-3", "ooooxxx/oooxxxx/ooo1xxx/o5x/7/7/7 x"),
]


def search(net, pos, K, VL, seconds, dtype):
    """One timed search as uai.Searcher runs it, with every iteration's tree and tower launches timed."""
    target = min(uai.Searcher.TIME_CAP_VISITS * K, uai.Searcher.MAX_VISITS)
    cfg = link.Config(games=1, visits=target + (1 if K == 1 else 0), max_plies=400, edges_per_node=96, c_puct=1.0,
                      dirichlet_alpha=0.15, dirichlet_weight=0.0, start_turn=pos.turn, seed=random.getrandbits(63),
                      start_x=pos.x, start_o=pos.o, blockers=0, flags=link.FLAG_TIE_FIRST | link.FLAG_PY_POSTERIOR)
    eng = link.Engine(cfg)
    if K > 1:
        eng.set_leaf_batch(K, VL)
    eng.timing_reset(1)
    start = time.time()
    eng.run(net, 1, dtype)
    rv, iters = 0, 1
    while rv < target and time.time() - start < seconds:
        chunk = 64 if K == 1 else min(16, -(-(target - rv) // K))
        if K == 1:
            chunk = min(chunk, target - rv)
        eng.run(net, chunk, dtype)
        iters += chunk
        now = eng.game_state(0).root_visits
        if now == rv:
            break
        rv = now
    eng.sync()
    elapsed = time.time() - start
    tm = eng.timing()
    coll = eng.collisions()
    steps = eng.stats()["steps"]
    eng.close()
    return dict(visits=rv, seconds=elapsed, iterations=iters, tree_ms=tm["select_ms"] / max(tm["iterations"], 1),
                tower_ms=tm["net_ms"] / max(tm["iterations"], 1), collisions=coll, paths=steps, capped=rv >= target)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--movetime-ms", type=int, default=1000)
    ap.add_argument("--ks", default="1,8,16,32,48,64")
    ap.add_argument("--virtual-loss", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    link.require_gpu()
    conv, bn = model.random_init(12, 128, seed=1, perturb_bn=True)
    net = link.Net(conv, bn)
    dtype = link.DTYPE_F16
    ks = [int(k) for k in a.ks.split(",")]
    lines = ["# tools/uai_nps.py: go movetime %d ms, 12x128 net, f16, virtual loss %d, one engine per search"
             % (a.movetime_ms, a.virtual_loss),
             "# columns: position K visits/s  iterations  tree ms/it  tower ms/it  collisions/path  capped  ratio-to-K1"]
    search(net, uai.Position.from_fen(POSITIONS[0][1]), 1, 1, 0.2, dtype)  # warm-up (code objects, allocations)
    for name, fen in POSITIONS:
        pos = uai.Position.from_fen(fen)
        base = None
        for K in ks:
            r = search(net, pos, K, a.virtual_loss, a.movetime_ms * 1e-3, dtype)
            nps = r["visits"] / r["seconds"]
            base = nps if K == 1 else base
            line = "%-6s K=%-3d %9.0f visits/s  %6d it  tree %.4f  tower %.4f  coll %.3f  %s  x%.2f" % (
                name, K, nps, r["iterations"], r["tree_ms"], r["tower_ms"], r["collisions"] / max(r["paths"], 1),
                "capped" if r["capped"] else "-", nps / base if base else float("nan"))
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
