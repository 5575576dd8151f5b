"""Plain numpy restatement of the proof layer of the leaf-parallel search ("Proven wins and losses"), on top of
tests/vl_reference.py, whose arrays-in / arrays-out style it keeps.

A node is DECIDED if it is a finished position (result bits in info word 1, as ever) or if it was PROVEN: a proven node
keeps its edges and its result bits 0, and carries its value — the bits of +1.0f (the side to move there wins) or -1.0f
(it loses) — in info word 3, where a finished position carries its terminal value and every other node a 0.

select() is vl_reference.select with one more way for a path to end: at a decided node that is not the root (TERMINAL;
the backup then uses the node's value like a finished position's).  backup() is vl_reference.backup followed by the proof
rule, applied in path order to the TERMINAL paths whose last node became decided in this batch (a finished position the
batch created: node id >= b.nodes0; hitting a position settled earlier proves nothing new): from the parent X of the path's last node upwards, X is a proven win
if some child of X is decided with value -1, a proven loss if every edge of X has a child and every child is decided with
value +1; when X becomes proven the walk goes on with X's parent, otherwise (or when X was decided already) it stops.
(An EVAL path ends at a node that has just been created, which is never decided: it proves nothing.)  Proofs only set
marks: W and n are vl_reference's.
"""
import ctypes

import numpy as np

from oracle import oracle_lib as orc
from tests import helpers
from tests import vl_reference as vlr

NONE = vlr.NONE
LEAF_NONE, LEAF_EVAL, LEAF_TERMINAL, LEAF_ROOT, LEAF_COLLISION = (vlr.LEAF_NONE, vlr.LEAF_EVAL, vlr.LEAF_TERMINAL,
                                                                  vlr.LEAF_ROOT, vlr.LEAF_COLLISION)
WIN_BITS, LOSS_BITS, is_proven = vlr.WIN_BITS, vlr.LOSS_BITS, vlr.is_proven


def decided_value(info_row):
    """+1 / -1 for a decided node (finished or proven), seen from its side to move; 0 for an undecided one."""
    w = int(info_row[3])
    if (int(info_row[1]) >> 16) == 0 and w not in (WIN_BITS, LOSS_BITS):
        return 0
    return 1 if w == WIN_BITS else -1


def select(tree, root_visits, visits, K, VL, c_puct, tie_first, blockers, node_cap=None, edge_cap=None):
    """vl_reference.select in which every proven node but the root ends a path like a finished position."""
    return vlr.select(tree, root_visits, visits, K, VL, c_puct, tie_first, blockers, node_cap, edge_cap,
                      proven_end_paths=True)


def prove(b):
    """The proof rule after a batch's backup.  Sets info word 3 of the nodes it proves in b.info and returns them in the
    order they were proven: [(node, value, path, levels above the path's last node)]."""
    out = []
    for p, path in enumerate(b.paths):
        if b.kind[p] != LEAF_TERMINAL or not path or b.leaf_node[p] < b.nodes0:
            continue
        nodes = [0] + [b.child[e] for e in path]
        for d in range(len(path) - 1, -1, -1):
            x = nodes[d]
            if decided_value(b.info[x]) != 0:
                break
            first, m = b.info[x][0], b.info[x][1] & 0xFFFF
            vals = [decided_value(b.info[b.child[e]]) if b.child[e] != NONE else None for e in range(first, first + m)]
            if any(v == -1 for v in vals):
                value = 1
            elif m > 0 and all(v == 1 for v in vals):
                value = -1
            else:
                break
            b.info[x][3] = WIN_BITS if value == 1 else LOSS_BITS
            out.append((x, value, p, len(path) - d))
    return out


def backup(b, values):
    """-> (edges (m, 4) u32, root visits added, proven [(node, value, path, levels)]); b.info carries the new marks."""
    edges, added = vlr.backup(b, values)
    return edges, added, prove(b)


def expected_tree(b, values, post_tree):
    """The whole dump after the backup and its proofs (the priors of the batch's new edges from `post_tree`, as
    vl_reference.expected_tree) -> ((boards, info, edges, moves), root visits added, proven)."""
    proven = prove(b)
    tree, added = vlr.expected_tree(b, values, post_tree)
    return tree, added, proven


def finished_bits(tree):
    """Per edge: 1 where the device's edge record must carry the "finished" bit of its child's range (bit 31 of word 3 of
    azh_engine_tree_raw) — the child is decided — else 0."""
    boards, info, edges, moves = tree
    out = np.zeros(len(edges), dtype=np.uint32)
    for e in range(len(edges)):
        c = int(edges[e, 3])
        if c != NONE and decided_value(info[c]) != 0:
            out[e] = 1
    return out


def late_positions(max_empty, count=None):
    """Unfinished fixture positions with at most `max_empty` empty cells, emptiest boards last: [(packed, blockers)]."""
    out = []
    for packed, blockers, rec in helpers.fixture_positions():
        x, o = int(packed[0]) & ~(1 << 63), int(packed[1])
        empty = 49 - bin(x | o | blockers).count("1")
        if empty > max_empty:
            continue
        p = orc.pos_from_fen(rec["fen"])
        p.blockers = blockers
        if orc.result(p) != 0:
            continue
        out.append((empty, int(packed[0]), int(packed[1]), blockers))
    out = sorted(set(out))
    return [(a, b, c) for _, a, b, c in out][:count]


class _OutOfBudget(Exception):
    pass


def _search(p, depth, memo, budget):
    """+1 / -1 for the side to move, or None if `depth` plies do not decide it.  A decided value does not depend on the
    depth it was found with, so it is remembered under the position alone."""
    pos = (int(p.pieces[0]), int(p.pieces[1]), int(p.turn))
    if pos in memo:
        return memo[pos]
    if (pos, depth) in memo:
        return None
    budget[0] -= 1
    if budget[0] < 0:
        raise _OutOfBudget()
    moves = np.zeros(256, dtype=np.uint16)
    m = ctypes.c_int(0)
    res = orc.lib().orc_result(ctypes.byref(p), moves.ctypes.data, ctypes.byref(m))
    if res != 0:
        out = 1 if (res == 1) == (p.turn == 0) else -1
    elif depth == 0:
        out = None
    else:
        out, open_ = -1, False
        for mv in sorted((int(v) for v in moves[:m.value]), key=lambda v: (v & 0xFF) != (v >> 8)):   # clones first
            q = orc.Pos()
            ctypes.memmove(ctypes.byref(q), ctypes.byref(p), ctypes.sizeof(orc.Pos))
            orc.lib().orc_makemove(ctypes.byref(q), mv & 0xFF, mv >> 8)
            v = _search(q, depth - 1, memo, budget)
            if v == -1:
                out = 1
                break
            open_ = open_ or v is None
        if out == -1 and open_:
            out = None
    if out is None:
        memo[(pos, depth)] = None
    else:
        memo[pos] = out
    return out


def _minimax(p, depth, memo, nodes=4000):
    """Plain minimax on the oracle's rules to the end of the game or `depth` plies, deepened ply by ply; gives up (None:
    not resolved) after `nodes` positions.  What it does return is exact."""
    budget = [nodes]
    try:
        for d in range(min(1, depth), depth + 1):
            v = _search(p, d, memo, budget)
            if v is not None:
                return v
    except _OutOfBudget:
        pass
    return None


def _pos(word0, word1, blockers):
    p = orc.Pos()
    p.pieces[0], p.pieces[1], p.blockers, p.turn = int(word0) & ~(1 << 63), int(word1), int(blockers), int(word0) >> 63
    return p
