"""tools/anchor_match.py, a net against the device's alpha-beta player on one engine: every move is legal, the anchor's moves
are the restatement's best moves, results and the printed table follow from the game lines, every opening is played both
ways."""
import json

import numpy as np
import pytest

from ataxxzero_amd import link, model
from tests import alphabeta_reference as ab
from tests import rules_reference as rr
from tools import anchor_match

pytestmark = pytest.mark.gpu

GAMES, VISITS, DEPTH, OPENING = 8, 16, 1, 4
_cache = {}


def match():
    if "games" not in _cache:
        conv, bn = model.random_init(2, 64, seed=5, perturb_bn=True)
        net = link.Net(conv, bn, model.BN_EPSILON)
        try:
            _cache["games"] = anchor_match.play_match(net, VISITS, DEPTH, GAMES, opening_depth=OPENING, seed=3)
        finally:
            net.close()
    return _cache["games"]


def cells_board(cells, turn):
    """the 49 cells of a game line (index x + 7 y, y = 0 at rank 7) -> restated board"""
    return rr.Board([cells[sq % 7 + 7 * (6 - sq // 7)] for sq in range(49)], turn)


def test_moves_are_legal_the_anchor_plays_best_and_results_follow():
    games = match()
    assert len(games) == GAMES
    anchor_plies = 0
    for g in games:
        assert len(g["boards"]) == len(g["moves"]) > 0
        b = cells_board(g["boards"][0], OPENING % 2)
        for cells, text in zip(g["boards"], g["moves"]):
            assert b.reference_cells() == cells
            assert rr.result(b) == 0
            move = rr.move_from_string(text)
            assert move in rr.legal_moves(b)
            if (b.turn == 0) != g["net_is_x"]:
                assert move == ab.search(b, DEPTH)[0], b.fen()
                anchor_plies += 1
            b = rr.make_move(b, move)
        assert g["result"] == rr.result(b) != 0
    assert anchor_plies > GAMES  # (a random net at 16 visits soon loses its few stones to a greedy capturer: the games are short)


def test_both_colours_for_every_opening():
    games = match()
    for k in range(GAMES // 2):
        a, b = games[2 * k], games[2 * k + 1]
        assert a["boards"][0] == b["boards"][0] and a["net_is_x"] and not b["net_is_x"]
        # the side to move after the opening is the net in one game and the anchor in the other
        first = cells_board(a["boards"][0], OPENING % 2)
        anchor_first = a if OPENING % 2 == 0 and not a["net_is_x"] or OPENING % 2 == 1 and a["net_is_x"] else b
        assert rr.move_from_string(anchor_first["moves"][0]) == ab.search(first, DEPTH)[0]
    assert len({json.dumps(g["boards"][0]) for g in games}) > 1


def test_the_printed_table_is_a_recount_of_the_game_lines(capsys):
    games = match()
    text, score = anchor_match.table(games)
    won = sum(1 for g in games if g["result"] == (1 if g["net_is_x"] else 2))
    lost = sum(1 for g in games if g["result"] == (2 if g["net_is_x"] else 1))
    assert won + lost == GAMES and score == won / GAMES
    lines = text.splitlines()
    for line, is_x in zip(lines, (True, False)):
        mine = [g for g in games if g["net_is_x"] == is_x]
        w = sum(1 for g in mine if g["result"] == (1 if is_x else 2))
        assert line.split() == ["net", "as", "xo"[not is_x] + ":", str(len(mine)), "games", str(w), "wins", str(len(mine) - w),
                                "losses", "0", "undecided"]
    assert lines[2].endswith("%.4f" % score)


def test_refused_combinations():
    for kwargs in ({"games": 7}, {"visits": 0}, {"visits": 60000}, {"start_fen": "7/7/7/7/7/7/7 x"}):
        args = dict(net=None, visits=VISITS, depth=DEPTH, games=GAMES)
        args.update(kwargs)
        with pytest.raises(ValueError):
            anchor_match.play_match(**args)
    conv, bn = model.random_init(2, 64, seed=5, perturb_bn=True)
    net = link.Net(conv, bn, model.BN_EPSILON)
    try:
        with pytest.raises(link.AzhError):
            anchor_match.play_match(net, VISITS, 9, GAMES)   # the search refuses the depth
        with pytest.raises(link.AzhError):
            anchor_match.play_match(net, VISITS, 4, GAMES)   # and depth 4 without a budget
    finally:
        net.close()
