"""The one restated descent (tests/vl_reference.py::select) under its two options, on the CPU, over trees the oracle grew:
scored by tests/exploration_reference.py with the mode's values off it is the plain descent, with them on its first edge is
the pick of scores() over the root's rows, and a path that reaches a node marked proven ends there."""
import numpy as np
import pytest

from oracle import oracle_lib as orc
from tests import exploration_reference as xr
from tests import helpers
from tests import solver_reference as sr
from tests import vl_reference as vlr
from tests.test_vl_reference import UAI, _fixture_fens

PARAMS = [(0.25, 0.0, 0.0), (-1.0, 19652.0, 1.25), (0.25, 19652.0, 1.25)]     # tests/test_gpu_exploration.py's three
_TREES = {}


def _trees(flags):
    """[(tree, root visits, cfg)]: every fourth search iteration of four fixture positions, 80 visits each."""
    if flags not in _TREES:
        out = []
        for fen in _fixture_fens(4):
            cfg = orc.make_config(games=1, visits=80, seed=7, fen_str=fen)
            cfg.flags, cfg.edges_per_node = flags, 96
            if flags:
                cfg.dirichlet_weight = 0.0
            oe = orc.Engine(cfg)
            for it in range(85):
                st = oe.game_state(0)
                if st.phase == 2:
                    break
                if st.phase == 1 and it % 4 == 0:
                    out.append((oe.tree(0), st.root_visits, cfg))
                oe.select()
                oe.backup(*helpers.synthetic_evals_distinct(oe.leaf_boards()))
            oe.close()
        _TREES[flags] = out
    return _TREES[flags]


def _args(tree, rv, cfg, K, VL):
    return tree, rv, cfg.visits, K, VL, cfg.c_puct, bool(cfg.flags & 2), cfg.blockers


@pytest.mark.parametrize("flags", [UAI, 0])
def test_with_the_mode_off_and_nothing_proven_it_is_the_plain_descent(flags):
    trees = _trees(flags)
    assert len(trees) >= 60
    for tree, rv, cfg in trees:
        args = _args(tree, rv, cfg, 7, 3)
        plain, explored = vlr.select(*args), xr.select(*args, *xr.OFF)
        for field in ("kind", "leaf_edge", "leaf_node", "leaf_board", "paths"):
            assert getattr(plain, field) == getattr(explored, field), field
        assert explored.proven_hits == 0


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("flags", [UAI, 0])
def test_the_first_edge_is_the_pick_of_the_scores_over_the_roots_rows(flags, params):
    differs = 0
    for tree, rv, cfg in _trees(flags):
        args = _args(tree, rv, cfg, 1, 1)
        first, M = int(tree[1][0][0]), int(tree[1][0][1]) & 0xFFFF
        rows = tree[2][first:first + M]
        n = [int(v) for v in rows[:, 1]]
        sc = xr.scores(rows[:, 0].copy().view(np.float32), rows[:, 2].copy().view(np.float32), n, sum(n), cfg.c_puct, *params)
        b = xr.select(*args, *params)
        assert b.paths[0][0] == first + vlr.pick(sc, bool(flags & 2))
        differs += b.paths[0] != vlr.select(*args).paths[0]
    assert differs > 0      # (the mode is not a no-op on these trees)


@pytest.mark.parametrize("flags", [UAI, 0])
def test_a_path_that_reaches_a_node_marked_proven_ends_there(flags):
    met = 0
    for tree, rv, cfg in _trees(flags):
        args = _args(tree, rv, cfg, 1, 1)
        plain = vlr.select(*args)
        if len(plain.paths[0]) < 2:
            continue                # the first edge's child is new, or finished: nothing to mark
        node = int(tree[2][plain.paths[0][0]][3])
        info = tree[1].copy()
        info[node][3] = vlr.LOSS_BITS
        marked = (tree[0], info, tree[2], tree[3])
        rest = args[1:]
        for b in (sr.select(marked, *rest), xr.select(marked, *rest, *xr.OFF), xr.select(marked, *rest, *PARAMS[1])):
            if b.paths[0][0] != plain.paths[0][0]:
                continue            # (the growing rate took another edge at the root)
            assert b.kind == [vlr.LEAF_TERMINAL] and b.leaf_node == [node] and b.paths[0] == plain.paths[0][:1]
            assert b.proven_hits == 1 and len(b.boards) == len(tree[0])          # nothing was expanded
            met += 1
        assert vlr.select(marked, *args[1:]).paths == plain.paths               # without the option the mark ends nothing
    assert met >= 60
