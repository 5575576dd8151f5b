"""The memoised restatement of the alpha-beta search's definition (tests/alphabeta_memo.py: integer masks, value and plain
node count remembered per position and depth) held to the cell-list negamax (tests/alphabeta_reference.py), and the deep
fixture (tests/golden/alphabeta_deep.json.gz) held to the memoised restatement and to the conditions the device tests lean on.
No device."""
import pytest

from tests import alphabeta_cases as ac
from tests import alphabeta_memo as am
from tests import alphabeta_reference as ab
from tests import rules_reference as rr

SAMPLE_EVERY = 5  # of the fixture's roots, recomputed to depth 8; every "forced" root besides


@pytest.mark.parametrize("name", [n for n, _, _ in ac.cases()])
def test_memo_equals_the_cell_list_negamax_on_the_named_cases(name):
    board, depth = next((b, d) for n, b, d in ac.cases() if n == name)
    for d in range(1, depth + 1):
        assert am.search(board, d) == ac.restated(name)[d - 1], (name, board.fen(), d)


def test_memo_equals_the_cell_list_negamax_on_the_deep_roots_to_depth_4():
    for root in ac.deep():
        for d in range(1, 5):
            want = ab.search(root.board, d)
            assert am.search(root.board, d) == want, (root.board.fen(), d)
            assert root.answers[d - 1] == want, (root.board.fen(), d)


def test_masks_restate_the_rules_of_the_cell_list():
    for root in ac.deep():
        b = root.board
        x, o, walls = b.masks()
        own, opp = (x, o) if b.turn == 0 else (o, x)
        assert am.result(own, opp, b.turn, walls) == rr.result(b)
        kids = am.children(own, opp, walls)
        assert [m for m, _, _ in kids] == rr.legal_moves(b)
        for m, mine, theirs in kids:
            c = rr.make_move(b, m)
            assert c.masks() == ((mine, theirs, walls) if b.turn == 0 else (theirs, mine, walls))


def test_the_fixture_is_what_the_memo_computes():
    roots = ac.deep()
    sample = [r for i, r in enumerate(roots) if i % SAMPLE_EVERY == 0 or r.family == "forced"]
    assert len(sample) >= len(roots) // SAMPLE_EVERY and len({r.region for r in sample}) == len({r.region for r in roots})
    for walls in sorted({r.board.masks()[2] for r in sample}):
        for r in sample:
            if r.board.masks()[2] == walls:
                assert am.all_depths(r.board, 8) == r.answers, r.board.fen()
                if r.family != "finished":
                    assert [am.pruned_nodes(r.board, d) for d in range(1, 9)] == r.pruned, r.board.fen()
        am.forget(walls)  # a 12-cell region leaves some 600 k entries


def test_a_textbook_alpha_beta_enters_no_more_than_the_plain_negamax_and_no_less_than_the_root_has_moves():
    for r in ac.deep():
        live = r.family != "finished"
        assert all(live * rr.count_moves(r.board) <= p <= a[2] for p, a in zip(r.pruned, r.answers)), r.board.fen()
        assert r.pruned[:2] == [a[2] for a in r.answers[:2]]  # one and two plies cannot be pruned: the last ply is searched whole


def test_the_deep_set_covers_what_the_device_tests_assume():
    roots = ac.deep()
    live = [r for r in roots if r.family != "finished"]
    assert len(live) >= 64 and all(rr.result(r.board) == 0 for r in live)
    assert all(rr.result(r.board) != 0 and r.answers[7][0] == ab.NO_MOVE for r in roots if r.family == "finished")
    assert all(bin(r.board.masks()[2]).count("1") >= 49 - 12 for r in roots)  # regions of at most 12 live cells
    assert len({r.board.masks()[2] for r in roots}) >= 7 and {r.board.turn for r in live} == {0, 1}
    # every win and loss value a depth-8 search can report: rem = 0 .. 7 below an unfinished root (a forced win or loss in
    # exactly 8 - rem plies), rem = 8 at a finished one
    at8 = {r.answers[7][1] for r in live}
    assert {s * (ab.WIN + rem) for s in (1, -1) for rem in range(8)} <= at8
    assert {r.answers[7][1] for r in roots if r.family == "finished"} == {ab.WIN + 8, -(ab.WIN + 8)}
    assert any(abs(v) < ab.WIN for v in at8)
    # a faster win is preferred: somewhere the value rises from a material score to a win, or a win gets nearer, with depth
    assert any(abs(r.answers[d][1]) >= ab.WIN > abs(r.answers[d - 1][1]) for r in live for d in range(5, 8))
    assert any(r.answers[7][0] != r.answers[d][0] for r in live for d in range(4, 7))  # the best move still changes deep down
    assert max(r.answers[7][2] for r in live) > 10 ** 7  # trees a cell-list negamax could not restate
