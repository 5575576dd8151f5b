"""The leaf-parallel restatement (tests/vl_reference.py) on the CPU: with K = 1 it is the oracle's search, iteration by
iteration; on hand-built trees it shows virtual loss, collisions, terminal paths and truncation."""
import numpy as np
import pytest

from oracle import oracle_lib as orc
from tests import helpers
from tests import vl_reference as vlr

UAI = 1 | 2 | 4  # NO_REUSE | TIE_FIRST | PY_POSTERIOR


def _fixture_fens(count):
    recs = helpers.load_gz("rules_noblock.json.gz")
    fens = [r["fen"] for r in recs if orc.result(orc.pos_from_fen(r["fen"])) == 0]
    step = max(1, len(fens) // count)
    return fens[::step][:count]


@pytest.mark.parametrize("flags", [UAI, 0])
def test_k1_restatement_is_the_oracle_search(flags):
    iterations = 0
    for fen in _fixture_fens(4):
        cfg = orc.make_config(games=1, visits=80, seed=7, fen_str=fen)
        cfg.flags = flags
        cfg.edges_per_node = 96
        if flags:
            cfg.dirichlet_weight = 0.0
        oe = orc.Engine(cfg)
        for _ in range(90):
            st = oe.game_state(0)
            pre = oe.tree(0)
            _, need = oe.select()
            if st.phase != 1:
                lb = oe.leaf_boards()
                logits, values = helpers.synthetic_evals_distinct(lb)
                oe.backup(logits, values)
                continue
            b = vlr.select(pre, st.root_visits, cfg.visits, 1, 1, cfg.c_puct, bool(flags & 2), cfg.blockers)
            s2 = oe.game_state(0)
            assert b.kind[0] == s2.leaf_kind and b.leaf_node[0] == s2.leaf_node and len(b.paths[0]) == s2.path_len
            lb = oe.leaf_boards()
            if b.kind[0] == vlr.LEAF_EVAL:
                assert tuple(int(v) for v in lb[0]) == b.leaf_board[0]
            logits, values = helpers.synthetic_evals_distinct(lb)
            oe.backup(logits, values)
            post = oe.tree(0)
            (eb, ei, ee, em), added = vlr.expected_tree(b, values, post)
            assert (eb == post[0]).all() and (ei == post[1]).all() and (ee == post[2]).all() and (em == post[3]).all()
            assert oe.game_state(0).root_visits == st.root_visits + added
            iterations += 1
        oe.close()
    assert iterations >= 250


def _toy_tree(priors, visits, W, children_of_1=None, terminal_child=None):
    """Root with len(priors) edges (start position moves are irrelevant: only children matter)."""
    p = orc.pos_from_fen(orc.START_FEN_PLAIN)
    root = (int(p.pieces[0]), int(p.pieces[1]))
    M = len(priors)
    boards = [root]
    info = [[0, M, 0, 0]]
    edges = [[vlr._bits(pr), v, vlr._bits(w), vlr.NONE] for pr, v, w in zip(priors, visits, W)]
    moves = list(orc.movegen(p)[:M])
    if terminal_child is not None:
        boards.append(root)
        info.append([0, 1 << 16, 0, vlr._bits(np.float32(1.0))])
        edges[terminal_child][3] = 1
    return (np.array(boards, np.uint64), np.array(info, np.uint32), np.array(edges, np.uint32), np.array(moves, np.uint16))


def test_virtual_loss_spreads_paths_over_edges():
    # two equal edges: without virtual loss every path would take the same one (first max); with it they alternate
    tree = _toy_tree([0.5, 0.5, 0.0], [0, 0, 0], [0.0, 0.0, 0.0])
    b = vlr.select(tree, 0, 100, 4, 1, 1.0, True, 0)
    assert b.kind[:2] == [vlr.LEAF_EVAL, vlr.LEAF_EVAL]
    assert b.paths[0] == [0] and b.paths[1] == [1]
    # the third and fourth paths meet the two new (unevaluated) nodes: collisions, which keep their virtual loss
    assert b.kind[2:] == [vlr.LEAF_COLLISION, vlr.LEAF_COLLISION]
    edges, added = vlr.backup(b, [0.5, -0.5, 0.0, 0.0])
    assert added == 2 and list(edges[:3, 1]) == [1, 1, 0]


def test_terminal_paths_back_up_the_terminal_value_and_ties_follow_the_flag():
    tree = _toy_tree([0.9, 0.1], [1, 1], [0.0, 0.0], terminal_child=0)
    b = vlr.select(tree, 2, 100, 2, 1, 1.0, False, 0)
    assert b.kind[0] == vlr.LEAF_TERMINAL and b.paths[0] == [0]
    edges, added = vlr.backup(b, [0.0] * len(b.kind))
    # a terminal value of +1 for the side to move at the child is a score of 0 for the mover at the root
    assert edges[0, 1] == 1 + sum(1 for k, p in zip(b.kind, b.paths) if p[0] == 0 and k != vlr.LEAF_COLLISION)
    assert vlr.pick(np.array([1.0, 1.0], np.float32), True) == 0 and vlr.pick(np.array([1.0, 1.0], np.float32), False) == 1


def test_last_batch_is_truncated_at_the_visit_budget():
    tree = _toy_tree([0.3, 0.3, 0.4], [3, 3, 3], [1.0, 1.0, 1.0])
    b = vlr.select(tree, 9, 12, 64, 2, 1.0, True, 0)
    assert len(b.kind) == 3
    b = vlr.select(tree, 12, 12, 64, 2, 1.0, True, 0)
    assert len(b.kind) == 1  # at least one path, as the one-leaf search


def test_a_full_arena_drops_the_path_ends_the_batch_and_forces_the_move():
    # the start position's first three moves; every child has 16 replies: the edge arena holds the root's 3 and one child's 16
    tree = _toy_tree([0.5, 0.3, 0.2], [0, 0, 0], [0.0, 0.0, 0.0])
    free = vlr.select(tree, 0, 100, 4, 2, 1.0, True, 0)
    assert len(free.kind) == 4 and not free.over and free.kind[:3] == [vlr.LEAF_EVAL] * 3
    b = vlr.select(tree, 0, 100, 4, 2, 1.0, True, 0, node_cap=10, edge_cap=3 + 16 + 15)
    assert b.over and b.kind == [vlr.LEAF_EVAL, vlr.LEAF_NONE]          # the batch ends with the dropped path
    assert b.leaf_edge == [0, 1] and b.paths[1] == [1] and b.leaf_board[1] == (0, 0)
    assert b.leaf_node[1] == 0 and len(b.boards) == 2 and len(b.n) == 19 and b.child[1] == vlr.NONE   # nothing was added
    edges, added = vlr.backup(b, [0.25, 0.0])
    assert added == 1 and list(edges[:3, 1]) == [1, 0, 0] and edges[1, 2] == 0    # no visit, no score, no virtual loss left
    assert vlr.move_is_due(b, added, 100) and not vlr.move_is_due(free, 3, 100) and vlr.move_is_due(free, 100, 100)
    # the node arena: no room for any node -> the first path is dropped; a finished child needs a node, too
    b = vlr.select(tree, 0, 100, 4, 2, 1.0, True, 0, node_cap=1, edge_cap=1000)
    assert b.over and b.kind == [vlr.LEAF_NONE] and b.leaf_edge == [0]
    # with room for everything the caps change nothing
    b = vlr.select(tree, 0, 100, 4, 2, 1.0, True, 0, node_cap=10, edge_cap=1000)
    assert b.kind == free.kind and b.paths == free.paths and not b.over


def test_the_forced_move_is_the_draw_proportional_to_the_root_visits():
    tree = _toy_tree([0.5, 0.3, 0.2], [0, 0, 0], [0.0, 0.0, 0.0])
    assert vlr.forced_move(tree, 0, 7, 0, 0) == (0, int(tree[3][0]))     # a root without a visit: its first edge
    tree = _toy_tree([0.5, 0.3, 0.2], [0, 5, 0], [0.0, 0.0, 0.0])
    assert all(vlr.forced_move(tree, 5, 7, uid, ply)[0] == 1 for uid in range(4) for ply in range(4))
    tree = _toy_tree([0.5, 0.3, 0.2], [1, 0, 3], [0.0, 0.0, 0.0])
    picks = [vlr.forced_move(tree, 4, 7, uid, ply)[0] for uid in range(8) for ply in range(8)]
    assert set(picks) == {0, 2} and picks.count(2) > picks.count(0)
