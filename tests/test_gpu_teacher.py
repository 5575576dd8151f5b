"""Teacher games from the device's alpha-beta search (azh_alphabeta_play, generate_games.py --supervised-depth): the training
move of every traced ply is the restatement's best move, the move played is replaced exactly where the host Philox says so,
the boards follow under the restated rules, and the generator writes lines the trainer reads.  Depth 2 on the whole board
against the cell-list negamax; depths 3 and 4 on walled 12-cell regions against the memoised one (tests/alphabeta_memo.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import link, supervised, training
from tests import alphabeta_cases as ac
from tests import alphabeta_memo as am
from tests import alphabeta_reference as ab
from tests import rules_reference as rr
from tests.samples_fixtures import philox

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES, DEPTH, PLIES, SEED = 64, 2, 40, 0x1234_5678_9ABC_DEF1
STREAM_TEACHER = 9
SCHEDULE = link.teacher_thresholds(supervised.OPENING_RANDOMIZATION_SCHEDULE)
_cache = {}


def play(thresholds, fen=ac.START, starts=None):
    x, o, blockers = rr.Board.from_fen(fen).masks()
    return link.alphabeta_play(GAMES, SEED, x, o, blockers, 0, DEPTH, 0, thresholds, PLIES, starts)


def scheduled():
    if "scheduled" not in _cache:
        _cache["scheduled"] = play(SCHEDULE)
    return _cache["scheduled"]


def best(b):
    """the restatement's best(b, DEPTH), once per position"""
    key = (b.fen(), b.masks()[2])
    if key not in _cache:
        _cache[key] = ab.search(b, DEPTH)[0]
    return _cache[key]


def check_games(trace, thresholds, walls, first=None, sample_every=7, best=best):
    """everything but the search: boards follow the moves played, moves are replaced where Philox says, results; the
    training move of every `sample_every`-th (game, ply) is restated by `best`"""
    plies, results, boards, training_moves, played = trace
    replaced = 0
    for g in range(len(plies)):
        b = first[g] if first is not None else rr.Board.from_fen(ac.START)
        wall = walls[g] if np.ndim(walls) else walls
        for p in range(int(plies[g])):
            assert (int(boards[g, p, 0]), int(boards[g, p, 1]), wall) == b.masks(), (g, p)
            assert rr.result(b) == 0
            legal = rr.legal_moves(b)
            t, m = int(training_moves[g, p]), int(played[g, p])
            v = philox(SEED, g, p, STREAM_TEACHER, 0)
            if p < len(thresholds) and v[0] < int(thresholds[p]):
                assert m == legal[(v[1] * len(legal)) >> 32], (g, p)
                replaced += m != t
            else:
                assert m == t, (g, p)
            assert t in legal
            if (g * PLIES + p) % sample_every == 0:
                assert t == best(b), (g, p, b.fen())
            b = rr.make_move(b, m)
        assert results[g] == rr.result(b), g
        assert plies[g] == PLIES or results[g] != 0
        assert not boards[g, int(plies[g]):].any() and not played[g, int(plies[g]):].any()
    return replaced


def test_training_moves_played_moves_boards_and_results():
    # one (game, ply) in 37, every ply among them: a depth-2 restatement costs some 2.5 k nodes in the middle game
    replaced = check_games(scheduled(), SCHEDULE, 0, sample_every=37)
    assert replaced >= 10  # the schedule's 10 plies at 20 % .. 4 % over 64 games: some 55 replacements expected
    plies = scheduled()[0]
    assert (plies == PLIES).any() or (scheduled()[1] != 0).all()


def test_without_thresholds_the_teacher_plays_its_own_moves():
    for thresholds in ((), np.zeros(10, dtype=np.uint32)):
        plies, results, boards, training_moves, played = play(thresholds)
        assert (training_moves == played).all()
    # every game is then the same game: the search has no randomness of its own
    assert (boards == boards[0]).all() and (plies == plies[0]).all()
    check_games((plies, results, boards, training_moves, played), (), 0, sample_every=3)  # (some 14 distinct positions)


def test_a_full_threshold_on_ply_0_makes_every_first_move_the_random_one():
    thresholds = np.array([2 ** 32 - 1], dtype=np.uint32)
    plies, results, boards, training_moves, played = play(thresholds)
    legal = rr.legal_moves(rr.Board.from_fen(ac.START))
    first = [legal[(philox(SEED, g, 0, STREAM_TEACHER, 0)[1] * len(legal)) >> 32] for g in range(GAMES)]
    assert played[:, 0].tolist() == first and len(set(first)) > 4
    assert (training_moves[:, 0] == ab.search(rr.Board.from_fen(ac.START), DEPTH)[0]).all()
    assert (training_moves[:, 1:] == played[:, 1:]).all()


def test_a_start_and_a_wall_map_per_game():
    fens = [ac.START, ac.WALLED_START, "x5o/7/7/7/7/7/o5x o", ac.LOST]
    first = [rr.Board.from_fen(fens[g % len(fens)]) for g in range(GAMES)]
    packed = np.array([b.packed() for b in first], dtype=np.uint64)
    walls = [b.masks()[2] for b in first]
    trace = play(SCHEDULE, starts=(packed, np.array(walls, dtype=np.uint64)))
    check_games(trace, SCHEDULE, walls, first, sample_every=61)
    assert (trace[0][3::4] < 10).all() and (trace[1][3::4] != 0).all()  # the lost position (two empty squares) is soon over
    assert (trace[2][2::4, 0, 0] == packed[2, 0] & np.uint64((1 << 49) - 1)).all()  # o moves first where the start says so


def region_start(f0, r0, w, h, turn):
    """the four-corner start of a w x h region whose lowest cell is (file f0, rank r0), every other cell a wall"""
    cells = [f + 7 * r for r in range(r0, r0 + h) for f in range(f0, f0 + w)]
    corner = lambda f, r: 1 << (f0 + f + 7 * (r0 + r))  # noqa: E731
    return rr.Board.from_masks(corner(0, 0) | corner(w - 1, h - 1), corner(w - 1, 0) | corner(0, h - 1),
                               (1 << 49) - 1 - sum(1 << c for c in cells), turn)


@pytest.mark.parametrize("depth", [3, 4])
def test_teacher_games_at_depths_3_and_4_in_walled_regions(depth):
    """16 games on 12-cell regions, four placements and so four wall words, either side first: every training move of
    every ply against the memoised restatement at the depth played (generate_games.py recommends depth 3).  The budget is
    beyond every position's plain count of depths 1 .. 4 (at most some 10 k there), so no iteration is abandoned."""
    places = ((0, 0, 3, 4), (4, 3, 3, 4), (2, 2, 4, 3), (3, 0, 4, 3))
    first = [region_start(*places[g % 4], (g // 4) % 2) for g in range(16)]
    packed = np.array([b.packed() for b in first], dtype=np.uint64)
    walls = [b.masks()[2] for b in first]
    assert len(set(walls)) == 4
    trace = link.alphabeta_play(16, SEED, 0, 0, 0, 0, depth, 1 << 20, SCHEDULE, PLIES, (packed, np.array(walls, dtype=np.uint64)))
    seen = {}

    def memo_best(b):
        seen[b.fen()] = am.search(b, depth)
        return seen[b.fen()][0]

    check_games(trace, SCHEDULE, walls, first, sample_every=1, best=memo_best)
    print("depth %d: %d plies, %d distinct positions, %d games ended" % (depth, trace[0].sum(), len(seen), (trace[1] != 0).sum()))
    assert trace[0].sum() >= 64 and len(seen) >= 32 and (trace[1] != 0).any()
    assert max(n for _, _, n in seen.values()) < 1 << 18  # the budget was never near
    for walls_of_region in set(walls):
        am.forget(walls_of_region)


def run_generator(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "generate_games.py")] + list(argv), cwd=ROOT, capture_output=True,
                          timeout=300)


def test_generator_writes_lines_the_trainer_reads(tmp_path):
    path = str(tmp_path / "teacher.json")
    res = run_generator("--supervised-depth", "1", "--game-count", "8", "--output-games", path)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    lines = [l for l in open(path) if l.strip()]
    assert len(lines) == 8
    entries = training.load_entries([path])
    assert len(entries) == 8
    for entry in entries:
        assert list(entry) == ["boards", "moves", "result"] and entry["result"] in (1, 2)
        assert len(entry["boards"]) == len(entry["moves"]) > 0
    start = rr.Board.from_fen(ac.START)
    first = json.loads(lines[0])
    assert first["boards"][0] == start.reference_cells()
    # the first training move is the restatement's, in the engine's move format: f1, the clone onto (5, 6)
    assert first["moves"][0] == ["c", [5, 6]] and ab.search(start, 1)[0] == rr.move_from_string("f1")
    training.get_sample_from_entries(entries)


def test_generator_refuses_two_teachers():
    res = run_generator("--supervised-depth", "1", "--supervised", "some engine", "--no-write")
    assert res.returncode != 0 and b"two teachers" in res.stderr
    res = run_generator("--supervised-depth", "4", "--supervised-nodes", "0", "--no-write")
    assert res.returncode != 0 and b"--supervised-nodes" in res.stderr
