#!/usr/bin/env python3
"""Generate tests/golden/rules_edge.json.gz: positions that random play from the start never reaches, answered by the
reference's own Python rules.

Run in the build container only (needs /root/reference, which never travels), beside gen_rules_fixtures.py:

    PYTHONHASHSEED=0 python tests/golden/gen_rules_edge_fixtures.py

Imports `ataxx_rules` and `uai_interface` from /root/reference unmodified and writes one data-only file.  No test imports
this script.  Every choice of a position is made by this script (seeded `random.Random`, and for the wide boards a seeded
single-cell hill climb on the length of the reference's own `legal_moves()`); every ANSWER (moves, result, successors, perft
counts) is the reference's.  The record format is that of rules_noblock.json.gz (fen, to_move, sorted UAI moves or ["0000"],
result 0 / 1 / 2, the 49-cell board list, successor FENs) with two differences: `succ` holds EVERY successor, not a sample of
four, and each record names its blocker set and its family.

Blocker sets (the module constant ataxx_rules.BLOCKED_CELLS, as gen_rules_fixtures.py sets it):
  none    no blockers
  block4  the four self-play blockers
  block3  a1, c2, f5 = (1<<0)|(1<<9)|(1<<33): asymmetric, 46 playable squares, so a full board can be an exact tie
  wall8   the eight squares within two steps of a1: a stone on a1 can never move, and an empty a1 can never be filled

Families:
  random  cells drawn independently, over a grid of densities from nearly empty to nearly full (not game positions)
  few     one to three stones a side; a single stone on every playable square
  stuck   the side to move has no move while squares are still empty; the opponent can move ("stuck"), or cannot because
          the only empty square is the walled-in a1 ("stuck_both")
  full    no empty square, exact 23-23 ties under block3 among them
  near    one or two empty squares
  wide    more than 128 legal moves, found by the hill climb (its trail; o to move = the same boards with the colours swapped)
  capture a jump that flips eight stones, a move that leaves the opponent without a stone, a clone with several sources
and `perft`: depth 1-3 counts (perft.py semantics: a position without a move has one child, the pass) for 16 of the positions.

Left out: boards without any stone (the reference's result() asserts on them) and boards where the side to move is stuck and
its opponent has no stones: there the reference's Python result() (pass first: the empty squares go to the stoneless
opponent) and its C++ get_board_result (stones first: the side to move wins) disagree, the kernels follow the C++ order, and
tests/test_rules_reference.py covers those boards from the restatement instead.
"""
import array
import gzip
import json
import os
import random
import sys

sys.path.insert(0, "/root/reference")
import ataxx_rules  # noqa: E402
import uai_interface  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SETS = {
    "none": [],
    "block4": [(3, 2), (2, 3), (4, 3), (3, 4)],
    "block3": [(0, 6), (2, 5), (5, 2)],
    "wall8": [(x, y) for x in range(3) for y in range(4, 7) if (x, y) != (0, 6)],
}
DENSITIES = [0.03, 0.08, 0.15, 0.25, 0.35, 0.5, 0.65, 0.75, 0.85, 0.92, 0.97]


def set_blockers(cells):
    ataxx_rules.BLOCKED_CELLS = frozenset(cells)
    ataxx_rules.LEGAL_SQUARE_COUNT = ataxx_rules.SIZE * ataxx_rules.SIZE - len(cells)


def mask_of(cells):
    return sum(1 << (x + 7 * (6 - y)) for x, y in cells)


def playable():
    return [(x, y) for y in range(7) for x in range(7) if (x, y) not in ataxx_rules.BLOCKED_CELLS]


def state_of(stones, to_move):
    """stones: {(x, y): 1 or 2}"""
    s = ataxx_rules.AtaxxState(array.array("b", [0] * 49), to_move=to_move)
    for xy, v in stones.items():
        assert xy not in ataxx_rules.BLOCKED_CELLS and v in (1, 2)
        s[xy] = v
    return s


def stones_of(state):
    return {(x, y): state[x, y] for y in range(7) for x in range(7) if state[x, y]}


def swapped(state):
    return state_of({xy: 3 - v for xy, v in stones_of(state).items()}, 3 - state.to_move)


def is_stuck(state):
    return state.copy().legal_moves() == ["pass"]


def usable(state):
    """not one of the boards the docstring leaves out"""
    n1, n2 = state.board.count(1), state.board.count(2)
    if n1 == 0 and n2 == 0:
        return False
    other = n2 if state.to_move == 1 else n1
    return not (other == 0 and is_stuck(state))


def in_uai_order(moves):
    return sorted(moves, key=uai_interface.uai_encode_move)


def position_record(state, set_name, family):
    state = state_of(stones_of(state), state.to_move)  # a fresh object: no cached move list
    moves = state.legal_moves()
    rec = {
        "set": set_name,
        "family": family,
        "fen": state.fen(),
        "to_move": state.to_move,
        "moves": sorted(uai_interface.uai_encode_move(m) for m in moves),
        "result": state.result() or 0,
        "cells": list(state.board),
    }
    succ = {}
    for m in in_uai_order(moves):
        c = state.copy()
        c.move(m)
        succ[uai_interface.uai_encode_move(m)] = c.fen()
    rec["succ"] = succ
    return rec


def perft(state, depth):
    """-> (leaves, a pass occurs in the tree); perft.py:5-16 as a recursion"""
    if depth == 0:
        return 1, False
    total, passed = 0, False
    for m in state.copy().legal_moves():
        c = state.copy()
        c.move(m)
        n, p = perft(c, depth - 1)
        total += n
        passed = passed or p or m == "pass"
    return total, passed


def near(xy, d):
    x, y = xy
    return [(x + i, y + j) for i in range(-d, d + 1) for j in range(-d, d + 1)
            if (i, j) != (0, 0) and 0 <= x + i < 7 and 0 <= y + j < 7 and (x + i, y + j) not in ataxx_rules.BLOCKED_CELLS]


# ---------------------------------------------------------------- families

def fam_random(rng, per_density):
    out = []
    for d in DENSITIES:
        for i in range(per_density):
            q = rng.uniform(0.15, 0.85)
            stones = {xy: (1 if rng.random() < q else 2) for xy in playable() if rng.random() < d}
            out.append(state_of(stones, 1 + i % 2))
    return out


def fam_few(rng, n_random):
    out = []
    cells = playable()
    for i, xy in enumerate(cells):
        other = rng.choice([c for c in cells if c != xy])
        for to_move in (1, 2):
            out.append(state_of({xy: 1, other: 2}, to_move))
    for i in range(n_random):
        picks = rng.sample(cells, 6)
        a, b = rng.randint(1, 3), rng.randint(1, 3)
        stones = {xy: 1 for xy in picks[:a]}
        stones.update({xy: 2 for xy in picks[3:3 + b]})
        out.append(state_of(stones, 1 + i % 2))
    return out


def fam_stuck(rng, n):
    """the side to move is stuck, squares are still empty, the opponent can move"""
    out = []
    cells = playable()
    while len(out) < n:
        me = 1 + len(out) % 2
        seed = rng.choice(cells)
        mine = {seed}
        for _ in range(rng.randint(0, 4)):
            grow = [c for m in mine for c in near(m, 1) if c not in mine]
            if grow:
                mine.add(rng.choice(grow))
        stones = {xy: me for xy in mine}
        for m in mine:
            for c in near(m, 2):
                stones.setdefault(c, 3 - me)
        p_empty = rng.choice([0.1, 0.3, 0.6, 0.9])
        for c in cells:
            if c not in stones and rng.random() >= p_empty:
                stones[c] = 3 - me
        s = state_of(stones, me)
        if len(stones) == len(cells) or not is_stuck(s) or is_stuck(state_of(stones, 3 - me)):
            continue
        out.append(s)
    return out


def fam_stuck_both(rng, n):
    """wall8 only: a1 is the one empty square and nobody can reach it"""
    assert (0, 6) not in ataxx_rules.BLOCKED_CELLS and not near((0, 6), 2)
    out = []
    for i in range(n):
        q = rng.choice([0.3, 0.5, 0.5, 0.7])
        stones = {xy: (1 if rng.random() < q else 2) for xy in playable() if xy != (0, 6)}
        s = state_of(stones, 1 + i % 2)
        assert is_stuck(s) and is_stuck(state_of(stones, 3 - s.to_move))
        out.append(s)
    return out


def fam_full(rng, n, ties):
    out = []
    cells = playable()
    for i in range(n):
        q = rng.uniform(0.2, 0.8)
        out.append(state_of({xy: (1 if rng.random() < q else 2) for xy in cells}, 1 + i % 2))
    for i in range(ties):
        assert len(cells) % 2 == 0
        order = cells[:]
        rng.shuffle(order)
        s = state_of({xy: (1 if j < len(cells) // 2 else 2) for j, xy in enumerate(order)}, 1 + i % 2)
        assert s.board.count(1) == s.board.count(2)
        out.append(s)
    return out


def fam_near(rng, n):
    out = []
    cells = playable()
    for i in range(n):
        q = rng.uniform(0.2, 0.8)
        holes = rng.sample(cells, 1 + (i // 2) % 2)
        out.append(state_of({xy: (1 if rng.random() < q else 2) for xy in cells if xy not in holes}, 1 + i % 2))
    return out


def fam_wide(rng, restarts, keep_128, keep_170):
    """single-cell hill climb on len(legal_moves()), side 1 to move, both sides keeping at least one stone; keeps boards of
    the trail"""
    cells = playable()
    mid, top = [], []
    for _ in range(restarts):
        stones = {}
        for xy in cells:
            v = rng.choice((0, 0, 1, 2))
            if v:
                stones[xy] = v
        if len(set(stones.values())) < 2:
            continue
        n = len(state_of(stones, 1).legal_moves())
        improved = True
        while improved:
            improved = False
            order = [(xy, v) for xy in cells for v in (0, 1, 2)]
            rng.shuffle(order)
            for xy, v in order:
                old = stones.get(xy, 0)
                if v == old:
                    continue
                trial = dict(stones)
                trial.pop(xy, None)
                if v:
                    trial[xy] = v
                if len(set(trial.values())) < 2:
                    continue  # both sides keep a stone: without one the kernels adjudicate and list no move
                s = state_of(trial, 1)
                m = len(s.legal_moves()) if s.legal_moves() != ["pass"] else 0
                if m > n:
                    stones, n, improved = trial, m, True
                    if n > 170:
                        top.append(s)
                    elif n > 128:
                        mid.append(s)
    pick = lambda lst, k: [lst[(i * len(lst)) // k] for i in range(k)] if len(lst) > k else lst
    out = pick(mid, keep_128) + pick(top, keep_170)
    return [s if i % 2 == 0 else swapped(s) for i, s in enumerate(out)]


def fam_widest():
    """the widest board with a stone on each side that a longer run of the same climb has met: 193 moves"""
    rows = "oxxxxxx/......./......./xxxxxxx/xxxxxxx/......./....x.."
    s = state_of({(x, y): ".xo".index(c) for y, row in enumerate(rows.split("/")) for x, c in enumerate(row) if c != "."}, 1)
    assert len(s.legal_moves()) == 193
    return [s, swapped(s)]


def fam_capture(rng):
    out = []
    cells = playable()
    free = lambda c: all(n_ in cells for n_ in [(c[0] + i, c[1] + j) for i in (-1, 0, 1) for j in (-1, 0, 1)])
    centres = [c for c in cells if 1 <= c[0] <= 5 and 1 <= c[1] <= 5 and free(c)]
    for i, c in enumerate(rng.sample(centres, min(4, len(centres)))):
        me = 1 + i % 2
        # a jump into a hole ringed by eight enemy stones: all eight change sides
        ring2 = [x for x in near(c, 2) if x not in near(c, 1)]
        stones = {x: 3 - me for x in near(c, 1)}
        stones[rng.choice(ring2)] = me
        for x in rng.sample([x for x in cells if x not in stones and x != c], 5):
            stones[x] = rng.choice((1, 2))
        out.append(state_of(stones, me))
        # the move takes every stone the opponent has
        stones = {x: 3 - me for x in rng.sample(near(c, 1), rng.randint(1, 3))}
        far_free = [x for x in ring2 if x not in stones]
        stones[rng.choice(far_free)] = me
        spare = [x for x in near(c, 1) if x not in stones]
        if spare:
            stones[rng.choice(spare)] = me
        out.append(state_of(stones, me))
        # one clone destination, several stones that can make it
        stones = {x: me for x in rng.sample(near(c, 1), 4)}
        for x in rng.sample([x for x in cells if x not in stones and x != c], 6):
            stones[x] = 3 - me
        out.append(state_of(stones, me))
    return out


def dump_gz(name, obj):
    # mtime=0 keeps the archive byte-stable across regenerations.
    with gzip.GzipFile(os.path.join(HERE, name), "wb", mtime=0) as f:
        f.write(json.dumps(obj, separators=(",", ":")).encode())


def main():
    if os.environ.get("PYTHONHASHSEED") != "0":
        raise SystemExit("run as: PYTHONHASHSEED=0 python tests/golden/gen_rules_edge_fixtures.py (see the docstring)")
    positions, perfts = [], []
    plan = {  # per set: random boards per density, few-stone random boards, wide (restarts, >128, >170)
        "none": dict(per_density=6, few=40, wide=(6, 20, 10)),
        "block4": dict(per_density=5, few=40, wide=(2, 5, 0)),
        "block3": dict(per_density=5, few=40, wide=(3, 10, 4)),
        "wall8": dict(per_density=5, few=40, wide=(2, 5, 0)),
    }
    for k, (name, blocked) in enumerate(SETS.items()):
        set_blockers(blocked)
        rng = random.Random(20260 + k)
        p = plan[name]
        fams = [("random", fam_random(rng, p["per_density"])),
                ("few", fam_few(rng, p["few"])),
                ("stuck", fam_stuck(rng, 60)),
                ("stuck_both", fam_stuck_both(rng, 20) if name == "wall8" else []),
                ("full", fam_full(rng, 32, 12 if name == "block3" else 0)),
                ("near", fam_near(rng, 64)),
                ("wide", fam_wide(rng, *p["wide"]) + (fam_widest() if name == "none" else [])),
                ("capture", fam_capture(rng))]
        first = len(positions)
        for fam, states in fams:
            seen = set()
            for s in states:
                if not usable(s) or (s.fen() in seen):
                    continue
                seen.add(s.fen())
                positions.append(position_record(s, name, fam))
        # perft: four positions per set, small enough for depth 3 in Python; at least one per set with a pass inside the tree
        chosen = []
        for want_pass, fams_ in ((True, ("stuck", "near")), (False, ("few", "random")), (True, ("near", "stuck_both")),
                                 (False, ("capture", "random"))):
            for rec in positions[first:]:
                if rec["family"] not in fams_ or rec["fen"] in [c["fen"] for c in chosen]:
                    continue
                if not (want_pass or 8 <= len(rec["moves"]) <= 40):
                    continue
                s = state_of({(i % 7, i // 7): v for i, v in enumerate(rec["cells"]) if v}, rec["to_move"])
                counts = [perft(s, d) for d in (1, 2, 3)]
                if counts[2][1] != want_pass or (want_pass and counts[2][0] < 4):
                    continue
                chosen.append({"set": name, "fen": rec["fen"], "depth": {str(d + 1): c[0] for d, c in enumerate(counts)},
                               "pass_inside": counts[2][1]})
                break
        assert len(chosen) == 4, (name, chosen)
        perfts += chosen
    set_blockers(frozenset())
    sets = {name: {"cells": [list(c) for c in blocked], "mask": mask_of(blocked)} for name, blocked in SETS.items()}
    dump_gz("rules_edge.json.gz", {"sets": sets, "positions": positions, "perft": perfts})
    tally = {}
    for rec in positions:
        tally[rec["family"]] = tally.get(rec["family"], 0) + 1
    wide = [len(r["moves"]) for r in positions if r["family"] == "wide"]
    print(len(positions), "positions:", json.dumps(tally), "| wide > 128:", sum(n > 128 for n in wide),
          "> 170:", sum(n > 170 for n in wide), "max", max(wide),
          "| successors:", sum(len(r["succ"]) for r in positions),
          "| perft with a pass:", sum(p["pass_inside"] for p in perfts), "of", len(perfts),
          "| bytes:", os.path.getsize(os.path.join(HERE, "rules_edge.json.gz")))


if __name__ == "__main__":
    main()
