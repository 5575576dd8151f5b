"""Visits per second of the single-position search (uai.Searcher) with K leaves per iteration.

For K in --ks: a `go movetime` search (--movetime-ms) of a 12x128 net (random weights: the rate does not depend on them)
in f16 on the start position and three mid-game positions, each K in its own engine as uai.Searcher builds it.  Reported:
root visits per second, iterations, the HIP-event time per iteration of the tree launch and of the tower launch (every
iteration sampled), and collisions per path.  K = 1 is the one-leaf search exactly as uai.Searcher runs it.

    python tools/uai_nps.py [--movetime-ms 1000] [--ks 1,8,16,32,48,64] [--out profiles/FILE.txt]

--reuse-tree measures what keeping the tree across moves is worth instead: a fixed line of 16 plies (the engine's own
moves of one session at a fixed seed) is played through uai.Session at `go movetime 200` — `moves a b` + `go`, the
tree's owner moving every second ply — with and without --reuse-tree, K = 1 and K = 32.  Per `go`: inherited root
visits, new visits, wall time of the whole `go`; then the per-`go` overhead outside the search: a fresh engine + the
whole-tree copy (what every `go` costs without reuse) against the re-root + root report of the session engine.

    python tools/uai_nps.py --reuse-tree [--out profiles/uai_tree_reuse.txt]

--solver measures what the proof layer costs ("Proven wins and losses"): every (position, K) of --ks is searched
with the solver off and on, one after the other in the same process; the lines carry the proof counters.  With the solver
on K = 1 runs through the leaf-parallel kernel, so its off/on pair is also the one-leaf kernels against k_vl_tree.

    python tools/uai_nps.py --solver --ks 1,32 [--out profiles/uai_solver.txt]

--exploration R,B,C measures what first-play urgency and the growing exploration rate cost ("First-play urgency
and the exploration rate"): every (position, K) of --ks is searched with the mode off and with
azh_engine_set_exploration(R, B, C), --repeats times each, off and on in turn in the same process.  With the mode on K = 1
runs through the leaf-parallel kernel, as under the solver.  (Random weights: the rate is measured, not the strength.)

    python tools/uai_nps.py --exploration 0.25,19652,1.25 --ks 1,32 [--repeats 3] [--out profiles/FILE.txt]
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


def search(net, pos, K, VL, seconds, dtype, solver=False, exploration=None):
    """One timed search as uai.Searcher runs it, with every iteration's tree and tower launches timed."""
    target = min(uai.Searcher.TIME_CAP_VISITS * K, uai.Searcher.MAX_VISITS)
    cfg = link.Config(games=1, visits=target + (1 if K == 1 else 0), max_plies=400, edges_per_node=96, c_puct=1.0,
                      dirichlet_alpha=0.15, dirichlet_weight=0.0, start_turn=pos.turn, seed=random.getrandbits(63),
                      start_x=pos.x, start_o=pos.o, blockers=0, flags=link.FLAG_TIE_FIRST | link.FLAG_PY_POSTERIOR)
    eng = link.Engine(cfg)
    if K > 1:
        eng.set_leaf_batch(K, VL)
    if solver:
        eng.set_solver(True)
    if exploration:
        eng.set_exploration(*exploration)
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
        if solver and eng.root_proofs(0, 1)[0][0] != 0:   # as uai.Searcher: a timed search ends once the root is proven
            break
    eng.sync()
    elapsed = time.time() - start
    tm = eng.timing()
    coll = eng.collisions()
    steps = eng.stats()["steps"]
    proofs = eng.proof_stats()
    eng.close()
    return dict(proofs=proofs, visits=rv, seconds=elapsed, iterations=iters, tree_ms=tm["select_ms"] / max(tm["iterations"], 1),
                tower_ms=tm["net_ms"] / max(tm["iterations"], 1), collisions=coll, paths=steps, capped=rv >= target)


def _searcher(net_path, K, reuse):
    return uai.Searcher(net_path, dtype="f16", parallel_leaves=K, virtual_loss=1, reuse_tree=reuse)


def reuse_line(net_path, plies, seconds):
    """The fixed line: the moves a K = 1 reuse session plays against itself from the start position at seed 1."""
    random.seed(1)
    session = uai.Session(_searcher(net_path, 1, True))
    session.handle("uainewgame")
    line = []
    for _ in range(plies):
        out, _ = session.handle("go movetime %d" % int(seconds * 1000))
        move = out[-1].split()[1]
        if move == "0000":
            break
        line.append(move)
        session.handle("moves " + move)
    session.searcher.close()
    return line


def reference_openings(games, plies):
    """The first `plies` moves of the first `games` random-play games the reference wrote (tests/golden), as UAI text."""
    import gzip
    import json
    square = lambda xy: "abcdefg"[xy[0]] + str(7 - xy[1])
    out = []
    with gzip.open(os.path.join(ROOT, "tests", "golden", "random_play_games.jsonl.gz")) as f:
        for text in f.read().decode().split("\n")[:games]:
            moves = json.loads(text)["moves"][:plies]
            out.append([square(m[1]) if m[0] == "c" else square(m[0]) + square(m[1]) for m in moves])
    return out


def reuse_report(net, conv, bn, movetime_ms, out_path):
    import tempfile
    seconds = movetime_ms * 1e-3
    net_path = os.path.join(tempfile.mkdtemp(), "net.npy")
    model.save_model(net_path, conv, bn)
    fixed = [("own", reuse_line(net_path, 16, seconds))] + [("ref-%d" % i, line) for i, line in enumerate(reference_openings(2, 16))]
    lines = ["# tools/uai_nps.py --reuse-tree: go movetime %d ms, 12x128 net with RANDOM weights (a flat policy: the search's visits"
             % movetime_ms,
             "# spread over all replies, the least a kept tree can be worth), f16, virtual loss 1; one session per (line, K, reuse);",
             "# the engine is asked to move at every second ply of a fixed line, after `moves a b`.  Lines:"]
    lines += ["#   %-5s %s" % (name, " ".join(line)) for name, line in fixed]
    lines += ["# own: the moves a K = 1 reuse session played against itself at seed 1 (it ends when a side has no move);",
              "# ref-i: the first 16 plies of the i-th random-play game under tests/golden",
              "# columns: line  K  reuse  ply  inherited  new visits  root visits  go wall ms"]
    summary = []
    for K in (1, 32):
        for reuse in (False, True):
            inh = new = gos = 0
            wall = 0.0
            for name, line in fixed:
                random.seed(2)
                searcher = _searcher(net_path, K, reuse)
                session = uai.Session(searcher)
                session.handle("uainewgame")
                session.handle("go movetime 50")   # warm-up (allocations, code objects); the tree is dropped again
                session.handle("uainewgame")
                for ply in range(0, len(line), 2):
                    if ply:
                        session.handle("moves %s %s" % (line[ply - 2], line[ply - 1]))
                    t0 = time.time()
                    session.handle("go movetime %d" % movetime_ms)
                    dt = time.time() - t0
                    text = "%-5s K=%-3d reuse=%d ply %2d  inherited %6d  new %6d  root %6d  go %7.1f ms" % (
                        name, K, int(reuse), ply, searcher.last_inherited, searcher.last_steps,
                        searcher.last_inherited + searcher.last_steps, dt * 1e3)
                    print(text, flush=True)
                    lines.append(text)
                    inh += searcher.last_inherited
                    new += searcher.last_steps
                    wall += dt
                    gos += 1
                searcher.close()
            summary.append("summary K=%-3d reuse=%d  %d go  inherited %d  new %d  inherited share of root visits %.1f %%  "
                           "go wall %.1f ms mean (budget %d ms)" % (K, int(reuse), gos, inh, new, 100.0 * inh / max(inh + new, 1),
                                                                     wall / gos * 1e3, movetime_ms))
    # the per-go overhead outside the search, on trees of the size a 200 ms search leaves
    pos = uai.Position.initial()
    for K in (1, 32):
        fresh, copy, reroot, report = [], [], [], []
        for rep in range(5):
            t0 = time.time()
            target = min(uai.Searcher.TIME_CAP_VISITS * K, uai.Searcher.MAX_VISITS)
            eng = link.Engine(link.Config(games=1, visits=target + (1 if K == 1 else 0), max_plies=400, edges_per_node=96,
                                          c_puct=1.0, dirichlet_alpha=0.15, dirichlet_weight=0.0, start_turn=pos.turn, seed=1,
                                          start_x=pos.x, start_o=pos.o, blockers=0,
                                          flags=link.FLAG_TIE_FIRST | link.FLAG_PY_POSTERIOR))
            if K > 1:
                eng.set_leaf_batch(K, 1)
            eng.sync()
            t1 = time.time()
            eng.run(net, 1 + (1500 if K == 1 else 400), link.DTYPE_F16)
            eng.sync()
            t2 = time.time()
            eng.tree(0)
            t3 = time.time()
            rep_ = eng.root_report(0, 1)[0]
            t4 = time.time()
            eng.play_moves([int(rep_.pv[0])])
            t5 = time.time()
            nodes = eng.game_state(0).n_nodes
            eng.close()
            t6 = time.time()
            fresh.append((t1 - t0) + (t6 - t5))
            copy.append(t3 - t2)
            report.append(t4 - t3)
            reroot.append(t5 - t4)
        med = lambda v: sorted(v)[len(v) // 2] * 1e3
        summary.append("overhead K=%-3d per go, median of 5: engine create + destroy %.2f ms, whole-tree copy %.2f ms (root %d visits) | "
                       "re-root (play_moves, %d nodes kept) %.2f ms, root report %.2f ms"
                       % (K, med(fresh), med(copy), rep_.root_visits, nodes, med(reroot), med(report)))
    for text in summary:
        print(text, flush=True)
    lines += summary
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reuse-tree", action="store_true", help="measure tree reuse across the moves of a fixed line instead")
    ap.add_argument("--solver", action="store_true", help="every (position, K) with the proof layer off and on")
    ap.add_argument("--exploration", default=None, metavar="R,B,C",
                    help="every (position, K) with azh_engine_set_exploration(R, B, C) off and on")
    ap.add_argument("--repeats", type=int, default=3, help="searches per (position, K, off / on) with --exploration")
    ap.add_argument("--movetime-ms", type=int, default=1000)
    ap.add_argument("--ks", default="1,8,16,32,48,64")
    ap.add_argument("--virtual-loss", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    link.require_gpu()
    conv, bn = model.random_init(12, 128, seed=1, perturb_bn=True)
    net = link.Net(conv, bn)
    dtype = link.DTYPE_F16
    if a.reuse_tree:
        reuse_report(net, conv, bn, 200, a.out)
        return
    ks = [int(k) for k in a.ks.split(",")]
    lines = ["# tools/uai_nps.py: go movetime %d ms, 12x128 net, f16, virtual loss %d, one engine per search"
             % (a.movetime_ms, a.virtual_loss),
             "# columns: position K visits/s  iterations  tree ms/it  tower ms/it  collisions/path  capped  ratio-to-K1"]
    search(net, uai.Position.from_fen(POSITIONS[0][1]), 1, 1, 0.2, dtype)  # warm-up (code objects, allocations)
    if a.solver:
        lines[1] = "# columns: position K solver visits/s  iterations  tree ms/it  tower ms/it  proven nodes  proven hits  on/off"
        search(net, uai.Position.from_fen(POSITIONS[0][1]), 1, 1, 0.2, dtype, solver=True)
        for name, fen in POSITIONS:
            pos = uai.Position.from_fen(fen)
            for K in ks:
                off = None
                for on in (False, True):
                    r = search(net, pos, K, a.virtual_loss, a.movetime_ms * 1e-3, dtype, solver=on)
                    nps = r["visits"] / r["seconds"]
                    off = nps if not on else off
                    line = "%-6s K=%-3d solver=%d %9.0f visits/s  %6d it  tree %.4f  tower %.4f  proven %d  hits %d  x%.3f" % (
                        name, K, int(on), nps, r["iterations"], r["tree_ms"], r["tower_ms"], r["proofs"]["proven_nodes"],
                        r["proofs"]["proven_hits"], nps / off)
                    print(line, flush=True)
                    lines.append(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.exploration:
        params = tuple(float(v) for v in a.exploration.split(","))
        assert len(params) == 3, "--exploration takes fpu_reduction,c_base,c_init"
        lines[0] += "; exploration %g,%g,%g, %d searches each" % (params + (a.repeats,))
        lines[1] = "# columns: position K exploration visits/s  iterations  tree ms/it  tower ms/it  collisions/path  (last line of a pair: mean on / mean off)"
        search(net, uai.Position.from_fen(POSITIONS[0][1]), 1, 1, 0.2, dtype, exploration=params)
        for name, fen in POSITIONS:
            pos = uai.Position.from_fen(fen)
            for K in ks:
                rates = {False: [], True: []}
                for _ in range(a.repeats):
                    for on in (False, True):
                        r = search(net, pos, K, a.virtual_loss, a.movetime_ms * 1e-3, dtype, exploration=params if on else None)
                        nps = r["visits"] / r["seconds"]
                        rates[on].append(nps)
                        line = "%-6s K=%-3d exploration=%d %9.0f visits/s  %6d it  tree %.4f  tower %.4f  coll %.3f" % (
                            name, K, int(on), nps, r["iterations"], r["tree_ms"], r["tower_ms"], r["collisions"] / max(r["paths"], 1))
                        print(line, flush=True)
                        lines.append(line)
                mean = {on: sum(v) / len(v) for on, v in rates.items()}
                line = "%-6s K=%-3d off %9.0f (%.0f .. %.0f)  on %9.0f (%.0f .. %.0f) visits/s  x%.3f" % (
                    name, K, mean[False], min(rates[False]), max(rates[False]), mean[True], min(rates[True]), max(rates[True]),
                    mean[True] / mean[False])
                print(line, flush=True)
                lines.append(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
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
