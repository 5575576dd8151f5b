"""Match between search settings inside the device-resident loop ("Search settings per side"): two to sixteen
search sets, every set against every other with the colours swapped, thousands of games in flight on ONE engine, one net.

A set is what one side searches with: --set "visits=400,leaves=1,vl=1,cpuct=1.0,fpu=0.25,cpuct-base=19652,cpuct-init=1.25";
a key left out takes the reference search's value (400 visits, one leaf, virtual loss 1, c_puct 1, first-play urgency off, the
constant exploration rate).  Game uid is played by the sets link.search_set_pairing(uid, n) names: uids 2q and 2q + 1 are one
pairing with the colours swapped, and with the start pool's stride of 2 they share their opening — the position after
--opening-plies plies of a uniformly random game (tools.solver_match.openings).  --games is rounded up to a multiple of
n (n - 1), so that every ordered pair plays equally often.

The engine is built with the flags uai.Searcher plays with (first maximal move on a tie, the Python posterior, no root noise)
and a fresh tree per move unless --reuse-tree; the move of a ply is the device loop's own draw in proportion to the visits.
Per unordered pair (a, b) the table gives the games, each set's wins as x and as o, the undecided games (cut at the ply
limit), the score of set a over the decided games and its 95 % interval (Wilson).  The table is the device's tally
(Engine.search_set_stats); the tool recounts it from the games' records (uid and result) and fails if the two disagree or if
a record was lost.

WITH RANDOM WEIGHTS A MATCH SAYS NOTHING ABOUT THE SETTINGS: give a trained net with --network PATH (tools/learning_curve.py
writes one per generation); without it the tool plays --blocks x 128 random weights, which exercises the code path only.

    python tools/settings_match.py --network model.npy --set visits=400 --set visits=100 --set visits=400,fpu=0.25,cpuct-base=19652,cpuct-init=1.25
                                   [--games 2000] [--concurrent 1024] [--opening-plies 8] [--out profiles/FILE.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ataxxzero_amd import link, model, uai  # noqa: E402
from tools.exploration_match import wilson  # noqa: E402
from tools.solver_match import openings  # noqa: E402

# key of --set -> (field of link.SearchSet, type, the reference search's value)
KEYS = {"visits": ("visits", int, 400), "leaves": ("leaves", int, 1), "vl": ("virtual_loss", int, 1),
        "cpuct": ("c_puct", float, 1.0), "fpu": ("fpu_reduction", float, -1.0), "cpuct-base": ("c_base", float, 0.0),
        "cpuct-init": ("c_init", float, 0.0)}


def parse_set(text):
    """"visits=400,fpu=0.25" -> the dict Engine.set_search_sets takes"""
    out = {field: default for field, _, default in KEYS.values()}
    for item in filter(None, (t.strip() for t in text.split(","))):
        key, eq, value = item.partition("=")
        if not eq or key.strip() not in KEYS:
            raise ValueError("--set: %r is not one of %s=VALUE" % (item, ", ".join(KEYS)))
        field, kind, _ = KEYS[key.strip()]
        out[field] = kind(value)
    return out


def set_text(t):
    return ",".join("%s=%g" % (key, t[field]) for key, (field, _, _) in KEYS.items())


def recount(words, n):
    """The (n, n, 4) table from record words, markers of dropped games included: by uid and result alone."""
    table = np.zeros((n, n, link.SET_STAT_COUNT), dtype=np.uint64)
    for r in link.records(words, markers=True):
        x, o = link.search_set_pairing(r.uid, n)
        table[x, o, link.SET_STAT_GAMES] += 1
        column = {1: link.SET_STAT_X_WINS, 2: link.SET_STAT_O_WINS}.get(r.result, link.SET_STAT_UNDECIDED)
        if r.kind & link.REC_KIND_MASK == link.REC_KIND_DROPPED:
            column = link.SET_STAT_UNDECIDED
        table[x, o, column] += 1
    return table


def pair_rows(table):
    """One row per unordered pair -> [(a, b, games, a wins as x, a wins as o, b wins as x, b wins as o, undecided)]"""
    n = table.shape[0]
    rows = []
    for a in range(n):
        for b in range(a + 1, n):
            ab, ba = table[a, b], table[b, a]      # a is x; b is x
            rows.append((a, b, int(ab[0] + ba[0]), int(ab[1]), int(ba[2]), int(ba[1]), int(ab[2]), int(ab[3] + ba[3])))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--network", default=None, metavar="PATH", help=".npy weights of a trained net (without it: random weights)")
    ap.add_argument("--set", action="append", default=[], metavar="K=V,...", dest="sets", help="one search set (two to sixteen)")
    ap.add_argument("--games", type=int, default=2000)
    ap.add_argument("--concurrent", type=int, default=1024, help="games in flight")
    ap.add_argument("--opening-plies", type=int, default=8)
    ap.add_argument("--dtype", default="f16", choices=sorted(link.DTYPES))
    ap.add_argument("--solver", action="store_true", help="both sides with the proof layer on")
    ap.add_argument("--random-symmetry", action="store_true", help="every leaf under a random board symmetry")
    ap.add_argument("--reuse-tree", action="store_true", help="keep the subtree of the move played (built by the other side's set)")
    ap.add_argument("--max-plies", type=int, default=400)
    ap.add_argument("--blocks", type=int, default=2, help="depth of the random net (without --network)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not 2 <= len(a.sets) <= link.SEARCH_SETS_MAX:
        ap.error("give two to %d --set" % link.SEARCH_SETS_MAX)
    try:
        sets = [parse_set(t) for t in a.sets]
    except ValueError as err:
        ap.error(str(err))
    n = len(sets)
    per = n * (n - 1)
    games = -(-max(a.games, 1) // per) * per
    if games != a.games:
        print("--games %d rounded up to %d, a multiple of n (n - 1) = %d: every ordered pair plays %d games"
              % (a.games, games, per, games // per), flush=True)
    link.require_gpu()
    if a.network is None:
        print("WARNING: no --network: %dx128 RANDOM weights.  The result says NOTHING about the settings." % a.blocks,
              file=sys.stderr, flush=True)
        conv, bn = model.random_init(a.blocks, 128, seed=a.seed, perturb_bn=True)
        net_text = "%dx128 net with RANDOM weights (says nothing about the settings)" % a.blocks
    else:
        conv, bn = model.load_model(a.network)
        net_text = a.network
    net = link.Net(conv, bn, model.BN_EPSILON)
    pool = [(x, o, 0, turn) for x, o, turn in openings(games // 2, a.opening_plies, a.seed)]
    if not pool:
        sys.exit("settings_match: no opening of %d plies is still on" % a.opening_plies)
    start = uai.Position.initial()
    G = max(1, min(a.concurrent, games))
    K = max(t["leaves"] for t in sets)
    flags = link.FLAG_TIE_FIRST | link.FLAG_PY_POSTERIOR | (0 if a.reuse_tree else link.FLAG_NO_REUSE)
    cfg = link.Config(games=G, visits=max(t["visits"] for t in sets), max_plies=a.max_plies, edges_per_node=96, c_puct=1.0,
                      dirichlet_alpha=0.15, dirichlet_weight=0.0, start_turn=start.turn, seed=a.seed, start_x=start.x,
                      start_o=start.o, blockers=0, flags=flags)
    e = link.Engine(cfg)
    e.set_start_pool(pool, stride=2)
    if K > 1:
        e.set_leaf_batch(K, 1)
    if a.solver:
        e.set_solver(True)
    if a.random_symmetry:
        e.set_random_symmetry(True)
    e.set_search_sets(sets)
    e.set_game_limit(games)
    overflow0 = e.stats()["ring_overflow"]
    dtype = link.DTYPES[a.dtype]
    words, over, steps, t0 = [], 0, 0, time.time()
    chunk = max(8, min(256, min(t["visits"] for t in sets) // K + 2))
    while over < games:
        e.run(net, chunk, dtype)
        e.fetch()
        words.append(e.staged_records().copy())
        e.drain_json()
        st = e.stats()
        if st["ring_overflow"] != overflow0 or st["games"] + st["dropped"] + st["steps"] == over + steps:
            break    # a lost record, or a chunk in which nothing moved: reported below, never waited out
        over, steps = st["games"] + st["dropped"], st["steps"]
    wall = time.time() - t0
    table = e.search_set_stats()
    mine = recount(np.concatenate(words), n)
    moved = e.stats()["ring_overflow"] - overflow0
    e.close()
    lines = ["# tools/settings_match.py: %d games, %d in flight, openings of %d random plies shared by the two colourings of a "
             "pairing, %s, %s, solver %s, random symmetry %s, %s" % (games, G, a.opening_plies, net_text, a.dtype,
                                                                     "on" if a.solver else "off", "on" if a.random_symmetry else "off",
                                                                     "the tree kept across moves" if a.reuse_tree else "a fresh tree per move")]
    lines += ["# set %d: %s" % (i, set_text(t)) for i, t in enumerate(sets)]
    lines.append("# pair   games   a:x-wins a:o-wins   b:x-wins b:o-wins   undecided   score of a   95 % interval")
    for i, b, g, ax, ao, bx, bo, und in pair_rows(table):
        wins, decided = ax + ao, ax + ao + bx + bo
        lo, hi = wilson(wins, decided)
        lines.append("%2d-%-2d %7d   %8d %8d   %8d %8d   %9d   %10.3f   %.3f .. %.3f"
                     % (i, b, g, ax, ao, bx, bo, und, wins / max(decided, 1), lo, hi))
    lines.append("wall %.1f s, %.1f games/s" % (wall, games / max(wall, 1e-9)))
    print("\n".join(lines), flush=True)
    if moved:
        sys.exit("settings_match: the record ring overflowed (%d records lost): the table cannot be checked" % moved)
    if not (table == mine).all():
        sys.exit("settings_match: the device's tally disagrees with the records:\n%s\nrecords:\n%s" % (table, mine))
    if int(table[:, :, link.SET_STAT_GAMES].sum()) != games:
        sys.exit("settings_match: the tally holds %d games, not %d" % (int(table[:, :, 0].sum()), games))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
