"""A net against the device's alpha-beta player ("Alpha-beta search"): a fixed yardstick for a net's strength.

    python tools/anchor_match.py --network model.npy --visits 100 --depth 2 --games 200
                                 [--nodes N] [--opening-depth 4] [--start-fen FEN] [--dtype f16] [--out games.jsonl]

Every opening (arena.random_openings: --opening-depth uniformly random plies from the start position) is played both ways, and
all games are in flight at once on one single-net engine with a fresh tree per move (AZH_FLAG_NO_REUSE), loaded so that the
net is to move in every live slot: where the anchor moves first its move is applied before loading.  Per round every live
root is searched with --visits steps, the most visited root move (the first in move order on a tie) is played with
azh_engine_play_moves, then one azh_alphabeta_search call answers all live roots and its moves are played the same way; slots
whose game has ended drop out.  The table gives the net's wins and losses per colour and its score; --out writes one line
{"boards", "moves", "result", "net_is_x"} per game (boards: the position before each move as 49 cells; moves: UAI strings).

WITH RANDOM WEIGHTS A MATCH SAYS NOTHING: give a trained net with --network PATH; without it the tool plays --blocks x
--filters random weights, which exercises the code path only.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ataxxzero_amd import arena, link, model, selfplay  # noqa: E402

BOARD = (1 << 49) - 1


def table(games):
    """The printed table from game lines alone -> (text, score of the net over the decided games or None)"""
    rows, won, decided = [], 0, 0
    for colour, net_is_x in (("x", True), ("o", False)):
        mine = [g for g in games if g["net_is_x"] == net_is_x]
        wins = sum(1 for g in mine if g["result"] == (1 if net_is_x else 2))
        losses = sum(1 for g in mine if g["result"] == (2 if net_is_x else 1))
        rows.append("net as %s: %4d games  %4d wins  %4d losses  %4d undecided" % (colour, len(mine), wins, losses,
                                                                                  len(mine) - wins - losses))
        won += wins
        decided += wins + losses
    score = won / decided if decided else None
    rows.append("net's score over %d decided games: %s" % (decided, "%.4f" % score if decided else "-"))
    return "\n".join(rows), score


def play_match(net, visits, depth, games, nodes=0, opening_depth=0, start_fen=selfplay.START_FEN_PLAIN, dtype="f16", seed=1,
               max_plies=400):
    """-> the games, in slot order: slots 2k and 2k + 1 share opening k, the net is x in the even one"""
    if games < 2 or games % 2:
        raise ValueError("--games must be even and at least 2: every opening is played both ways")
    if visits < 1 or visits >= 60000:
        raise ValueError("--visits must be 1 .. 59999 (the engine's visit counts are 16 bits wide)")
    x, o, walls, turn = selfplay.parse_fen(start_fen)
    why = selfplay.start_refusal(x, o, walls, turn)
    if why:
        raise ValueError("--start-fen: " + why)
    if opening_depth > 0:
        openings, _ = arena.random_openings(games // 2, opening_depth, seed, start_fen)
    else:
        openings = np.array([[x | (turn << 63), o]] * (games // 2), dtype=np.uint64)
    boards = np.repeat(openings, 2, axis=0)
    out = [{"boards": [], "moves": [], "result": 0, "net_is_x": g % 2 == 0} for g in range(games)]
    live = np.ones(games, dtype=bool)

    def record(slots, moves):
        """the moves of `slots` go into their games and onto `boards`; -> nothing.  Games that end leave `live`."""
        for g, m in zip(slots, moves):
            w0, w1 = int(boards[g, 0]), int(boards[g, 1])
            out[g]["boards"].append(selfplay.board_cells(w0 & BOARD, w1))
            out[g]["moves"].append(arena.uai_move(int(m)))
        boards[slots] = link.makemove_batch(boards[slots], np.asarray(moves, dtype=np.uint16))
        _, _, results = link.rules_batch(boards[slots], walls)
        for g, r in zip(slots, results):
            if r != 0 or len(out[g]["moves"]) >= max_plies:
                out[g]["result"] = int(r)
                live[g] = False

    def anchor_moves(slots):
        if len(slots):
            record(slots, link.alphabeta_search(boards[slots], walls, depth, nodes, outputs=("moves",)).moves)

    # the anchor moves first where it has the colour to move
    net_to_move = np.array([(int(boards[g, 0]) >> 63 == 0) == out[g]["net_is_x"] for g in range(games)])
    anchor_moves(np.flatnonzero(~net_to_move))
    # visits + 1: no move ever comes due on the device; the host names every move
    cfg = link.Config(games=games, visits=visits + 1, max_plies=max_plies, edges_per_node=96, c_puct=1.0, dirichlet_alpha=0.15,
                      dirichlet_weight=0.0, start_turn=turn, seed=seed, start_x=x, start_o=o, blockers=walls,
                      flags=link.FLAG_NO_REUSE | link.FLAG_TIE_FIRST | link.FLAG_PY_POSTERIOR)
    engine = link.Engine(cfg)
    try:
        # (a game the anchor's first move ended keeps the opening in its slot, which is never read again)
        loaded = np.where(live[:, None], boards, np.repeat(openings, 2, axis=0))
        engine.set_positions(loaded, np.zeros(games, dtype=np.int32))
        while live.any():
            engine.run(net, 1 + visits, link.DTYPES[dtype])  # the roots' evaluation and `visits` steps
            reports = engine.root_report(0, games)
            slots = np.flatnonzero(live)
            picked = []
            for g in slots:
                r = reports[g]
                if len(r.moves) == 0:
                    raise RuntimeError("slot %d: a live root without a move" % g)
                picked.append(int(r.moves[int(np.argmax(r.visits))]))  # the first maximum: the first in edge order on a tie
            moves = np.full(games, link.NO_MOVE, dtype=np.uint16)
            moves[slots] = picked
            status = engine.play_moves(moves)
            if (np.asarray(status)[slots] <= 0).any():
                raise RuntimeError("the engine refused a move it reported: statuses %s" % np.asarray(status)[slots].tolist())
            record(slots, picked)
            slots = np.flatnonzero(live)
            anchor_moves(slots)
            moves = np.full(games, link.NO_MOVE, dtype=np.uint16)
            for g in slots:
                moves[g] = move_code(out[g]["moves"][-1])
            status = engine.play_moves(moves)
            if (np.asarray(status)[slots] <= 0).any():
                raise RuntimeError("the engine refused the anchor's move: statuses %s" % np.asarray(status)[slots].tolist())
    finally:
        engine.close()
    return out


def move_code(text):
    """UAI text -> u16 (from | to << 8)"""
    sq = lambda t: "abcdefg".index(t[0]) + 7 * (int(t[1]) - 1)  # noqa: E731
    return sq(text) * 257 if len(text) == 2 else sq(text[:2]) | (sq(text[2:]) << 8)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--network", default=None, metavar="PATH", help=".npy weights of a trained net (without it: random weights)")
    ap.add_argument("--visits", type=int, default=100)
    ap.add_argument("--depth", type=int, default=2, help="depth of the alpha-beta player, 1 .. 8")
    ap.add_argument("--nodes", type=int, default=None, help="its node budget per move (default: none up to depth 3, 100000 beyond)")
    ap.add_argument("--games", type=int, default=200)
    ap.add_argument("--opening-depth", type=int, default=4)
    ap.add_argument("--start-fen", default=selfplay.START_FEN_PLAIN)
    ap.add_argument("--dtype", default="f16", choices=sorted(link.DTYPES))
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="file the game lines are written to")
    a = ap.parse_args(argv)
    nodes = a.nodes if a.nodes is not None else (0 if a.depth <= link.ALPHABETA_UNBOUNDED_DEPTH else 100000)
    link.require_gpu()
    if a.network is None:
        print("WARNING: no --network: %dx%d RANDOM weights.  The result says NOTHING about strength." % (a.blocks, a.filters),
              file=sys.stderr, flush=True)
        conv, bn = model.random_init(a.blocks, a.filters, seed=a.seed, perturb_bn=True)
    else:
        conv, bn = model.load_model(a.network)
    net = link.Net(conv, bn, model.BN_EPSILON)
    try:
        games = play_match(net, a.visits, a.depth, a.games, nodes, a.opening_depth, a.start_fen, a.dtype, a.seed)
    except (ValueError, link.AzhError) as err:
        sys.exit("anchor_match: %s" % err)
    finally:
        net.close()
    if a.out:
        with open(a.out, "w") as f:
            for g in games:
                f.write(json.dumps(g) + "\n")
    print("net %s, %d visits, against alpha-beta depth %d (node budget %d): %d games"
          % (a.network or "RANDOM", a.visits, a.depth, nodes, len(games)))
    print(table(games)[0])
    return games


if __name__ == "__main__":
    main()
