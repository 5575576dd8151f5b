"""The device alpha-beta search (azh_alphabeta_search) against the plain negamax of tests/alphabeta_reference.py: the move is
the FIRST best one, the value and the reported depth are exact, the node count lies between the root's move count and the
plain negamax count.  Shapes: one root, a wave short of / exactly / one past a workgroup row of 64, several workgroups;
move lists past 64 and 128 entries; walls per root.  Depths 6 to 8 run on the deep set (small walled regions, restated by
tests/alphabeta_memo.py and kept in tests/golden/alphabeta_deep.json.gz): every stack row, every win value 1000 .. 1008,
budgets that abandon iterations 5 to 8, and a node count held to a textbook alpha-beta's."""
import collections

import numpy as np
import pytest

from ataxxzero_amd import link
from tests import alphabeta_cases as ac
from tests import alphabeta_reference as ab
from tests import rules_reference as rr
from tests.helpers import load_gz

pytestmark = pytest.mark.gpu

BUDGET = 1 << 22
_cache = {}


def pack(boards):
    return (np.array([b.packed() for b in boards], dtype=np.uint64).reshape(-1, 2),
            np.array([b.masks()[2] for b in boards], dtype=np.uint64))


def check_against_restatement(boards, out, depth, want=None):
    """every root's answer at the depth it reports; want[i]: its all_depths list, restated here where not given"""
    for i, b in enumerate(boards):
        done = int(out.depth_done[i])
        assert 1 <= done <= depth, b.fen()
        per_depth = want[i] if want is not None else ab.all_depths(b, done)
        move, value, _ = per_depth[done - 1]
        assert (int(out.moves[i]), int(out.values[i])) == (move, value), (b.fen(), done)
        plain = sum(n for _, _, n in per_depth[:min(done + 1, len(per_depth))])  # the completed iterations and the abandoned one
        assert rr.kernel_count(b) * (rr.result(b) == 0) <= int(out.nodes[i]) <= plain, (b.fen(), done)


def trace_pool():
    """300 unfinished positions of uniform-random device games, spread over the plies -> [board]"""
    if "pool" not in _cache:
        start = rr.Board.from_fen(ac.START)
        x, o, bl = start.masks()
        plies, _, boards, _ = link.random_play(32, 77, x, o, bl, 0, 400)
        rng = np.random.default_rng(5)
        pool = []
        while len(pool) < 300:
            g = int(rng.integers(32))
            p = int(rng.integers(int(plies[g])))
            pool.append(rr.Board.from_masks(int(boards[g, p, 0]), int(boards[g, p, 1]), 0, p % 2))
        _cache["pool"] = pool
        _cache["pool_depth1"] = [ab.all_depths(b, 1) for b in pool]
    return _cache["pool"], _cache["pool_depth1"]


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_the_named_positions_batched(depth):
    named = [(n, b) for n, b, d in ac.cases() if d >= depth]
    boards = [b for _, b in named]
    packed, walls = pack(boards)
    out = link.alphabeta_search(packed, walls, depth, 0 if depth <= 3 else BUDGET)
    assert (out.depth_done == depth).all()  # without a budget, or far below it, every iteration completes
    check_against_restatement(boards, out, depth, [ac.restated(n) for n, _ in named])
    if depth <= 3:
        wide = [n for n, _ in named].index("wide")
        assert int(out.values[wide]) == 999 + depth
    # the pruning ratio, for the record (printed, not asserted)
    plain = sum(sum(n for _, _, n in ac.restated(name)[:depth]) for name, _ in named)
    print("depth %d: device nodes %d, plain negamax %d" % (depth, int(out.nodes.sum()), plain))


def test_finished_roots_among_live_ones():
    boards = ac.finished_boards() + [rr.Board.from_fen(ac.START)]
    packed, walls = pack(boards)
    out = link.alphabeta_search(packed, walls, 3)
    for i, b in enumerate(boards):
        assert (int(out.moves[i]), int(out.values[i])) == ab.search(b, 3)[:2]
    assert out.depth_done.tolist() == [3, 3, 3] and out.nodes[:2].tolist() == [0, 0]


def test_positions_of_random_play_at_depths_1_and_2():
    pool, depth1 = trace_pool()
    packed, _ = pack(pool)
    out = link.alphabeta_search(packed, 0, 1)
    assert (out.depth_done == 1).all()
    check_against_restatement(pool, out, 1, depth1)
    assert (out.nodes == [rr.kernel_count(b) for b in pool]).all()  # depth 1 enters every child once
    sample = list(range(0, 300, 8))  # a depth-2 restatement costs some 2.5 k nodes per mid-game position
    out = link.alphabeta_search(packed[sample], 0, 2)
    assert (out.depth_done == 2).all()
    check_against_restatement([pool[i] for i in sample], out, 2)


def test_walls_per_root_mixed_with_none():
    data = load_gz("rules_edge.json.gz")
    boards = []
    for name in ("block4", "none", "block3", "wall8"):
        recs = [r for r in data["positions"] if r["set"] == name]
        boards += [rr.Board.from_fen(r["fen"], data["sets"][name]["mask"]) for r in recs[::max(len(recs) // 24, 1)][:24]]
    order = np.random.default_rng(2).permutation(len(boards))
    boards = [boards[i] for i in order]
    packed, walls = pack(boards)
    assert len(set(walls.tolist())) >= 4 and (walls == 0).any()
    out = link.alphabeta_search(packed, walls, 1)
    live = [i for i, b in enumerate(boards) if rr.result(b) == 0]
    assert len(live) > 48 and max(rr.kernel_count(boards[i]) for i in live) > 128
    check_against_restatement([boards[i] for i in live], link.AlphaBeta(*(f[live] for f in out)), 1)
    for i, b in enumerate(boards):
        if rr.result(b) != 0:
            assert (int(out.moves[i]), int(out.values[i]), int(out.nodes[i])) == ab.search(b, 1)
    # one wall word for every root is the same as that word per root
    same = [i for i in range(len(boards)) if walls[i] == walls[0]]
    one = link.alphabeta_search(packed[same], int(walls[0]), 2)
    per = link.alphabeta_search(packed[same], walls[same], 2)
    assert all((a == b).all() for a, b in zip(one, per))
    small = [i for i in live if rr.kernel_count(boards[i]) <= 40][:8]  # depth 2 where the restatement is cheap
    check_against_restatement([boards[i] for i in small], link.alphabeta_search(packed[small], walls[small], 2), 2)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_workgroup_and_grid_edges(n):
    pool, depth1 = trace_pool()
    packed, _ = pack(pool)
    if "whole" not in _cache:
        _cache["whole"] = link.alphabeta_search(packed, 0, 2)
    whole = _cache["whole"]
    first = link.alphabeta_search(packed[:n], 0, 1)
    check_against_restatement(pool[:n], first, 1, depth1[:n])
    perm = np.random.default_rng(n).permutation(n)
    out = link.alphabeta_search(packed[perm], 0, 2)
    for got, ref in zip(out, whole):
        assert (got == ref[perm]).all()  # a root's answer does not depend on where it stands in the batch


def test_output_pointers_omitted_one_at_a_time():
    pool, _ = trace_pool()
    packed, _ = pack(pool[:65])
    names = ("moves", "values", "depth_done", "nodes")
    full = link.alphabeta_search(packed, 0, 2)
    for skip in names:
        out = link.alphabeta_search(packed, 0, 2, outputs=[f for f in names if f != skip])
        for f in names:
            assert getattr(out, f) is None if f == skip else (getattr(out, f) == getattr(full, f)).all()
    none = link.alphabeta_search(packed, 0, 2, outputs=())
    assert all(v is None for v in none)


def test_a_node_budget_reports_the_last_completed_iteration():
    named = [(n, b) for n, b, d in ac.cases() if d >= 3]
    boards = [b for _, b in named]
    packed, walls = pack(boards)
    out = link.alphabeta_search(packed, walls, 3, 256)
    wide = [n for n, _ in named].index("wide")
    # depth 1 costs exactly 157 nodes; any correct depth 2 enters at least the 157 children again, and 314 > 256
    move, value, _ = ac.restated("wide")[0]
    assert (int(out.moves[wide]), int(out.values[wide]), int(out.depth_done[wide])) == (move, value, 1)
    assert 157 < int(out.nodes[wide]) <= 257 + link.MAX_MOVES
    check_against_restatement(boards, out, 3, [ac.restated(n) for n, _ in named])
    assert len(set(out.depth_done.tolist())) > 1  # some roots complete more than the wide one does


def test_refusals():
    packed, _ = pack([rr.Board.from_fen(ac.START)])
    for depth, budget in ((0, 0), (9, 1 << 20), (4, 0), (2, 255)):
        with pytest.raises(link.AzhError) as err:
            link.alphabeta_search(packed, 0, depth, budget)
        assert "error -2" in str(err.value)
    with pytest.raises(link.AzhError):
        link.alphabeta_search(packed, packed[0, 0], 1)  # walls on the x stones


# ---------------------------------------------------------------- depths 6 to 8: the deep set
# tests/golden/alphabeta_deep.json.gz: roots in walled regions of at most 12 cells, restated to depth 8 by
# tests/alphabeta_memo.py (tests/test_alphabeta_memo.py holds the file to it, without a device).

def deep_set():
    if "deep" not in _cache:
        roots = ac.deep()
        _cache["deep"] = (roots,) + pack([r.board for r in roots])
    return _cache["deep"]


def deep_run(depth):
    """the whole set in one batch, walls per root, under a budget that lets every iteration complete: the largest plain
    negamax count of that depth, which no sound pruned search reaches"""
    if ("deep run", depth) not in _cache:
        roots, packed, walls = deep_set()
        budget = max(r.answers[depth - 1][2] for r in roots)
        assert budget > max(sum(r.pruned[:depth]) for r in roots)  # (and a textbook alpha-beta stays far below it)
        _cache["deep run", depth] = link.alphabeta_search(packed, walls, depth, budget), budget
    return _cache["deep run", depth]


@pytest.mark.parametrize("depth", [6, 7, 8])
def test_the_deep_set_at_depths_6_to_8(depth):
    roots, packed, walls = deep_set()
    assert len(roots) >= 64 and len(set(walls.tolist())) >= 7
    out, _ = deep_run(depth)
    assert (out.depth_done == depth).all()
    # move, value and root move count <= nodes <= the plain negamax counts of d = 1 .. depth
    check_against_restatement([r.board for r in roots], out, depth, [r.answers[:depth] for r in roots])
    # the window goes down whole: no more nodes than a textbook alpha-beta in the same move order enters
    textbook = np.array([sum(r.pruned[:depth]) for r in roots], dtype=np.uint64)
    worst = int(np.argmax(out.nodes.astype(np.int64) - textbook.astype(np.int64)))
    assert (out.nodes <= textbook).all(), (roots[worst].board.fen(), int(out.nodes[worst]), int(textbook[worst]))
    print("depth %d: device nodes %d, textbook alpha-beta %d, plain negamax %d; win values met %s" % (
        depth, int(out.nodes.sum()), int(textbook.sum()), sum(sum(a[2] for a in r.answers[:depth]) for r in roots),
        sorted({int(v) for v in out.values if abs(int(v)) >= ab.WIN})))


def test_a_budget_abandons_iterations_past_the_fourth_deep_in_the_stack():
    """Budgets from the fixture's plain counts C_j (iterations 1 .. j summed): C_4, halfway to C_5, and C_5.  A sound pruned
    search enters no more than C_4 nodes in its first four iterations, so each budget lets them complete and whatever is
    abandoned is iteration 5, 6, 7 or 8, the loop standing two plies or more below the root nearly always.  (An interval
    [C_(d-1), moves * d) that would also force iteration d to be abandoned is empty on every root: C_(d-1) is far above it.
    That the budgets do abandon is asserted below, not assumed: a minimal alpha-beta tree of depth 8 alone has about twice
    the leaves a plain tree of depth 4 has.)"""
    roots, _, _ = deep_set()
    big = [r for r in roots if r.answers[7][2] >= 1 << 20][::3]
    assert len(big) >= 12
    abandoned_at, roots_abandoned = collections.Counter(), 0
    for r in big:
        packed, walls = pack([r.board])
        plain = np.cumsum([a[2] for a in r.answers]).tolist()
        textbook = np.cumsum(r.pruned).tolist()
        moves = rr.kernel_count(r.board)
        hit = False
        for budget in (plain[3], (plain[3] + plain[4]) // 2, plain[4]):
            assert budget >= link.MAX_MOVES
            out = link.alphabeta_search(packed, walls, 8, budget)
            done, nodes = int(out.depth_done[0]), int(out.nodes[0])
            assert 4 <= done <= 8, (r.board.fen(), budget)
            assert (int(out.moves[0]), int(out.values[0])) == r.answers[done - 1][:2], (r.board.fen(), budget, done)
            assert moves * done <= nodes <= budget + link.MAX_MOVES, (r.board.fen(), budget, done)
            assert (nodes > budget) == (done < 8), (r.board.fen(), budget, done)  # abandoned: the count passed the budget
            # the iterations a textbook alpha-beta completes inside the budget are completed
            assert done >= max(d for d in range(1, 9) if textbook[d - 1] <= budget), (r.board.fen(), budget, done)
            if done < 8:
                abandoned_at[done + 1] += 1
                hit = True
        roots_abandoned += hit
    print("iterations abandoned: %s; %d of %d roots" % (sorted(abandoned_at.items()), roots_abandoned, len(big)))
    assert 2 * roots_abandoned >= len(big)
    assert sum(abandoned_at.values()) >= len(big) and len(abandoned_at) >= 2  # at d >= 5 each, and not all at one depth


@pytest.mark.parametrize("n", [1, 3, 4, 5, 0])
def test_deep_answers_do_not_depend_on_the_batch_or_the_waves_beside(n):
    """4 roots share a workgroup, each wave on its own stack in LDS: the longest searches first, beside shorter ones"""
    roots, packed, walls = deep_set()
    whole, budget = deep_run(8)
    rng = np.random.default_rng(8)
    size = np.array([r.answers[7][2] for r in roots])
    perm = np.concatenate([rng.permutation(np.nonzero(size >= 1 << 20)[0]), rng.permutation(np.nonzero(size < 1 << 20)[0])])
    perm = perm[:n] if n else rng.permutation(len(roots))
    out = link.alphabeta_search(packed[perm], walls[perm], 8, budget)
    for i, j in enumerate(perm):
        assert (int(out.moves[i]), int(out.values[i]), int(out.depth_done[i])) == roots[j].answers[7][:2] + (8,), roots[j].board.fen()
    for got, ref in zip(out, whole):
        assert (got == ref[perm]).all()
