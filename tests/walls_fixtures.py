"""Games on boards with walls for the tests of the wall mask's way through the loop (tests/test_walls_host.py,
tests/walls_gpu_checks.py): played here with tests/rules_reference.py's rules by a seeded random player, written as the game
lines the generator writes with --record-blockers.  Nothing comes from the reference's code or from the engine."""
import random

import numpy as np

from ataxxzero_amd import link, selfplay, training
from tests import rules_reference as rr

DEFAULT_FEN = selfplay.START_FEN_SELFPLAY                 # the four walls of the self-play start: cells [17, 23, 25, 31]
ASYMMETRIC_FEN = "-x4o/2-4/7/2-4/6-/7/o5x x"               # walls on cells 0, 9, 23 and the edge cell 34: every symmetry moves them
ASYMMETRIC_CELLS = [0, 9, 23, 34]
PLAIN_FEN = selfplay.START_FEN_PLAIN


def policy_index(move):
    """A rules_reference move -> its flat policy index, through the trainer's own table."""
    return training._flat_policy_index(rr.move_string(move))


def play_game(fen, seed, max_plies=48, with_key=True):
    """One random game from `fen` -> (entry, [rules_reference.Board before every ply]).  A ply without a move is a "pass" with an
    empty target; every other ply's "dists" spreads random weights (multiples of 1/64: exact in f32) over up to 12 legal
    moves.  A game still running after max_plies goes to the side with more stones."""
    rng = random.Random(seed)
    board = rr.Board.from_fen(fen)
    walls = board.masks()[2]
    entry = {"boards": [], "dists": [], "moves": []}
    if with_key:
        entry["blockers"] = link.blockers_to_cells(walls)
    positions = []
    while rr.result(board) == 0 and len(positions) < max_plies:
        legal = rr.legal_moves(board)
        positions.append(board)
        entry["boards"].append(board.reference_cells())
        if not legal:
            entry["moves"].append("pass")
            entry["dists"].append({})
            board = rr.make_move(board, rr.PASS)
            continue
        chosen = rng.sample(legal, min(len(legal), rng.randint(1, 12)))
        cuts = sorted(rng.sample(range(1, 64), len(chosen) - 1))
        parts = [b - a for a, b in zip([0] + cuts, cuts + [64])]
        entry["dists"].append({rr.move_string(m): p / 64.0 for m, p in sorted(zip(chosen, parts))})
        move = rng.choice(legal)
        entry["moves"].append(rr.move_string(move))
        board = rr.make_move(board, move)
    outcome = rr.result(board)
    entry["result"] = outcome if outcome else (1 if board.count(rr.X) >= board.count(rr.O) else 2)
    return entry, positions


_GAMES = {}


def games(fen, count, with_key=True, first_seed=100):
    """`count` games from `fen`, played once per process -> [(entry, positions)]."""
    key = (fen, count, with_key, first_seed)
    if key not in _GAMES:
        _GAMES[key] = [play_game(fen, first_seed + g, with_key=with_key) for g in range(count)]
    return _GAMES[key]


def mixed_entries():
    """A walled game on the default map, an unwalled one without the key, two on the asymmetric map, one more on the default map
    and one unwalled: the masks change from game to game, and one run of two games shares a mask."""
    picks = [games(DEFAULT_FEN, 2)[0], games(PLAIN_FEN, 2, with_key=False)[0], games(ASYMMETRIC_FEN, 2)[0],
             games(ASYMMETRIC_FEN, 2)[1], games(DEFAULT_FEN, 2)[1], games(PLAIN_FEN, 2, with_key=False)[1]]
    return [e for e, _ in picks], [p for _, p in picks]


def mover_view(board):
    """-> (mover's stones, opponent's stones, walls) as bit masks."""
    x, o, walls = board.masks()
    return (o, x, walls) if board.turn else (x, o, walls)


def wall_plane(cells):
    """The [x][y][1] plane of the wall cells (index x + 7 y) as training.apply_symmetry takes it."""
    plane = np.zeros((7, 7, 1), dtype=np.float32)
    for c in cells:
        plane[c % 7, c // 7, 0] = 1.0
    return plane


def is_legal_text(board, text):
    """Is the UAI move `text` legal for the side to move of the rules_reference board?"""
    if text in ("pass", "0000"):
        return not rr.legal_moves(board)
    return rr.move_from_string(text) in rr.legal_moves(board)


def replay_legal(fen, moves):
    """Plays UAI `moves` from `fen` with rules_reference -> the index of the first illegal move, or None."""
    board = rr.Board.from_fen(fen)
    for i, text in enumerate(moves):
        if not is_legal_text(board, text):
            return i
        board = rr.make_move(board, rr.PASS if text in ("pass", "0000") else rr.move_from_string(text))
    return None
