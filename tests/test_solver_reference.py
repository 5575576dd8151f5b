"""The proof layer's restatement (tests/solver_reference.py) on the CPU: without a proven node it is vl_reference step for
step; on hand-built three-level trees the rule proves exactly the nodes it should; and on late fixture positions every
node it proves has the value a plain minimax on the oracle's rules finds."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_lib as orc
from tests import helpers
from tests import solver_reference as sr
from tests import vl_reference as vlr
from tests.solver_reference import _minimax, _pos, late_positions

F32 = np.float32


# ------------------------------------------------------------------ a search on the host alone

def root_tree(word0, word1, blockers):
    """One-node tree at a packed position, uniform priors."""
    p = orc.Pos()
    p.pieces[0], p.pieces[1], p.blockers, p.turn = int(word0) & ~(1 << 63), int(word1), int(blockers), int(word0) >> 63
    moves = np.zeros(256, dtype=np.uint16)
    m = ctypes.c_int(0)
    res = orc.lib().orc_result(ctypes.byref(p), moves.ctypes.data, ctypes.byref(m))
    assert res == 0
    M = m.value
    edges = np.zeros((M, 4), dtype=np.uint32)
    edges[:, 0] = vlr._bits(F32(1.0) / F32(M))
    edges[:, 3] = vlr.NONE
    return (np.array([[int(word0), int(word1)]], dtype=np.uint64), np.array([[0, M, 0, 0]], dtype=np.uint32), edges,
            moves[:M].copy())


def host_search(tree, blockers, visits, K, VL, select, backup):
    """Iterations of (select, synthetic evaluation, backup) on arrays alone.  The priors of new nodes are a fixed positive
    function of the move (the proof rule does not read them).  -> (tree, [proven per iteration], [Batch per iteration])."""
    rv, log, batches = 0, [], []
    while rv < visits:
        b = select(tree, rv, visits, K, VL, 1.0, True, blockers)
        _, values = helpers.synthetic_evals_distinct(np.array(b.leaf_board, dtype=np.uint64).reshape(-1, 2))
        out = backup(b, values)
        edges, added, proven = out if len(out) == 3 else (out[0], out[1], [])
        for n in range(len(tree[0]), len(b.boards)):
            first, M = b.info[n][0], b.info[n][1] & 0xFFFF
            raw = np.array([(int(b.moves[first + j]) * 40503 + 12345) % 1009 + 1 for j in range(M)], dtype=np.float32)
            if M:
                edges[first:first + M, 0] = (raw / raw.sum(dtype=np.float32)).view(np.uint32)
        tree = (np.array(b.boards, dtype=np.uint64).reshape(-1, 2), np.array(b.info, dtype=np.uint32).reshape(-1, 4), edges,
                np.array(b.moves, dtype=np.uint16))
        log.append(proven)
        batches.append(b)
        if added == 0:
            break
        rv += added
    return tree, log, batches


def test_without_a_proven_node_it_is_vl_reference_step_for_step():
    steps = 0
    for (w0, w1, blockers), K, VL in zip(late_positions(49)[-200::50], (1, 7, 16, 3), (1, 3, 2, 1)):
        tree = root_tree(w0, w1, blockers)
        rv = 0
        for _ in range(12):
            a = vlr.select(tree, rv, 60, K, VL, 1.0, True, blockers)
            b = sr.select(tree, rv, 60, K, VL, 1.0, True, blockers)
            assert (a.kind, a.leaf_edge, a.leaf_board, a.paths, a.leaf_node) == (b.kind, b.leaf_edge, b.leaf_board, b.paths, b.leaf_node)
            assert (a.boards, a.info, a.n, a.W, a.child, a.moves) == (b.boards, b.info, b.n, b.W, b.child, b.moves)
            _, values = helpers.synthetic_evals_distinct(np.array(b.leaf_board, dtype=np.uint64).reshape(-1, 2))
            ea, added_a = vlr.backup(a, values)
            eb, added_b, proven = sr.backup(b, values)
            assert (ea == eb).all() and added_a == added_b
            if proven:
                break   # from here on the two searches may differ: that is the feature
            assert a.info == b.info
            tree = (np.array(b.boards, dtype=np.uint64).reshape(-1, 2), np.array(b.info, dtype=np.uint32).reshape(-1, 4), eb,
                    np.array(b.moves, dtype=np.uint16))
            rv += added_b
            steps += 1
    assert steps >= 20


# ------------------------------------------------------------------ hand-built trees

WIN, LOSS = sr.WIN_BITS, sr.LOSS_BITS


def _batch(nodes, paths, nodes0=None):
    """nodes: [(children or None per edge, result, value bits)], node 0 the root; paths: lists of (node, edge slot) hops
    -> a Batch as select leaves it, every path TERMINAL."""
    b = vlr.Batch()
    b.info, b.child = [], []
    for kids, res, bits in nodes:
        b.info.append([len(b.child), len(kids) | (res << 16), 0, bits])
        b.child += [vlr.NONE if k is None else k for k in kids]
    b.paths = [[b.info[n][0] + j for n, j in hops] for hops in paths]
    b.kind = [vlr.LEAF_TERMINAL] * len(paths)
    b.leaf_node = [b.child[p[-1]] for p in b.paths]
    b.nodes0 = min(b.leaf_node) if nodes0 is None else nodes0   # by default every path's last node is new
    return b


def test_any_child_loses_proves_a_win():
    # root -> A -> (finished: its mover has lost | not expanded); the root's other edge is not expanded
    b = _batch([([1, None], 0, 0), ([2, None], 0, 0), ([], 1, LOSS)], [[(0, 0), (1, 0)]])
    assert sr.prove(b) == [(1, 1, 0, 1)]
    assert b.info[1][3] == WIN and b.info[0][3] == 0


def test_all_children_win_proves_a_loss_and_the_proof_chains_to_the_root():
    # A's two children are finished positions their movers have won: A is lost, so the root's mover wins by going there
    b = _batch([([1, None], 0, 0), ([2, 3], 0, 0), ([], 1, WIN), ([], 2, WIN)], [[(0, 0), (1, 1)]])
    assert sr.prove(b) == [(1, -1, 0, 1), (0, 1, 0, 2)]
    assert b.info[1][3] == LOSS and b.info[0][3] == WIN


def test_an_unexpanded_edge_blocks_a_loss_proof():
    b = _batch([([1], 0, 0), ([2, None], 0, 0), ([], 1, WIN)], [[(0, 0), (1, 0)]])
    assert sr.prove(b) == [] and b.info[1][3] == 0
    # and so does an expanded child that is not decided
    b = _batch([([1], 0, 0), ([2, 3], 0, 0), ([], 1, WIN), ([None], 0, 0)], [[(0, 0), (1, 0)]])
    assert sr.prove(b) == []


def test_path_order_matters_when_two_paths_prove_siblings():
    # A and B are each proven a win by their own path; the root is lost only once both are: the second path's walk sees
    # the first path's proof, so it is the one that proves the root
    nodes = [([1, 2], 0, 0), ([3, None], 0, 0), ([4, None], 0, 0), ([], 1, LOSS), ([], 1, LOSS)]
    b = _batch(nodes, [[(0, 0), (1, 0)], [(0, 1), (2, 0)]])
    assert sr.prove(b) == [(1, 1, 0, 1), (2, 1, 1, 1), (0, -1, 1, 2)]
    b = _batch(nodes, [[(0, 1), (2, 0)], [(0, 0), (1, 0)]])
    assert sr.prove(b) == [(2, 1, 0, 1), (1, 1, 1, 1), (0, -1, 1, 2)]
    # one path alone leaves the root open
    b = _batch(nodes, [[(0, 0), (1, 0)]])
    assert sr.prove(b) == [(1, 1, 0, 1)] and b.info[0][3] == 0


def test_a_decided_node_is_never_proven_again_and_the_walk_stops_there():
    b = _batch([([1], 0, 0), ([2, None], 0, WIN), ([], 1, LOSS)], [[(0, 0), (1, 0)]])
    assert sr.prove(b) == []   # A was proven before: its parent was tested then


def test_a_hit_of_a_position_settled_earlier_walks_nothing():
    nodes = [([1, None], 0, 0), ([2, None], 0, 0), ([], 1, LOSS)]
    assert sr.prove(_batch(nodes, [[(0, 0), (1, 0)]], nodes0=3)) == []
    assert sr.prove(_batch(nodes, [[(0, 0), (1, 0)]], nodes0=2)) == [(1, 1, 0, 1)]


def test_select_ends_a_path_at_a_proven_node_but_descends_from_a_proven_root():
    p = orc.pos_from_fen(orc.START_FEN_PLAIN)
    root = (int(p.pieces[0]), int(p.pieces[1]))
    moves = list(orc.movegen(p)[:2])
    # the root (itself marked proven) has two edges; edge 0 leads to A, proven lost for its mover, which still has an edge
    boards = np.array([root, root], dtype=np.uint64)
    info = np.array([[0, 2, 0, WIN], [2, 1, 0, LOSS]], dtype=np.uint32)
    edges = np.array([[vlr._bits(F32(0.9)), 1, vlr._bits(F32(1.0)), 1], [vlr._bits(F32(0.1)), 0, 0, vlr.NONE],
                      [vlr._bits(F32(1.0)), 0, 0, vlr.NONE]], dtype=np.uint32)
    tree = (boards, info, edges, np.array(moves + moves[:1], dtype=np.uint16))
    b = sr.select(tree, 1, 100, 1, 1, 1.0, True, 0)
    assert b.kind == [sr.LEAF_TERMINAL] and b.paths == [[0]] and b.leaf_node == [1] and b.proven_hits == 1
    assert b.info[1] == [2, 1, 0, LOSS]   # the mark select uses inside never leaves it
    out, added, proven = sr.backup(b, [0.0])
    # A's mover loses: a full point for the root's mover on the edge, nothing proven anew
    assert added == 1 and int(out[0, 1]) == 2 and vlr._f(int(out[0, 2])) == F32(2.0) and proven == []
    # vl_reference walks through A and expands its edge: the two differ exactly there
    assert vlr.select(tree, 1, 100, 1, 1, 1.0, True, 0).paths == [[0, 2]]


# ------------------------------------------------------------------ soundness against a minimax


def test_every_proof_agrees_with_a_minimax_on_late_positions():
    positions = late_positions(6)[:200]   # the 200 fullest boards: at most 6 empty cells, deepest endgames first
    assert len(positions) == 200
    resolved = checked = made = 0
    kinds = set()
    for i, (w0, w1, blockers) in enumerate(positions):
        memo = {}
        if _minimax(_pos(w0, w1, blockers), 8, memo) is None:
            continue
        resolved += 1
        K, VL = ((1, 1), (4, 1), (16, 3))[i % 3]
        tree, log, _ = host_search(root_tree(w0, w1, blockers), blockers, 120, K, VL, sr.select, sr.backup)
        for proven in log:
            for node, value, _, levels in proven:
                made += 1
                truth = _minimax(_pos(int(tree[0][node][0]), int(tree[0][node][1]), blockers), 8, memo)
                if truth is None:
                    continue   # deeper than the minimax looks: not counted
                assert truth == value, (i, node, value, truth)
                checked += 1
                kinds.add((value, levels > 1, node == 0))
    print("positions resolved by the minimax: %d of 200; proofs made on them: %d, checked: %d; kinds met: %s"
          % (resolved, made, checked, sorted(kinds)))
    assert resolved >= 100, resolved
    # A proven node lies below a root the minimax resolved within its budget, and its own proof is a subtree of a search
    # of 120 visits: the same budget should resolve most of them.  Half is the floor below which the comparison would
    # say little about the proofs that were made; and there is at least one checked proof per resolved position.
    assert 2 * checked >= made and checked >= resolved, (made, checked, resolved)
    assert {v for v, _, _ in kinds} == {1, -1} and any(c for _, c, _ in kinds) and any(r for _, _, r in kinds)
