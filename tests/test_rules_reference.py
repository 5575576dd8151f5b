"""The plain cell-list restatement of the rules (tests/rules_reference.py) against the two other statements there are: the
fixtures the reference's own Python rules wrote (rules_noblock, rules_block4 and the edge positions of rules_edge: tests/golden/
gen_rules_fixtures.py, gen_rules_edge_fixtures.py) and the C oracle (oracle/ataxx_rules_oracle.c).  No GPU: what the kernels are
compared with in tests/test_gpu_rules_edges.py has to agree with itself first."""
import json
import os

import numpy as np
import pytest

from oracle import oracle_lib as orc
from tests import rules_reference as rr
from tests.helpers import BLOCK3_MASK, BLOCK4_MASK, GOLDEN, load_gz, orc_pos, pocket_boards


def fixture_records(name):
    """[(record, blockers mask)]"""
    if name == "edge":
        data = load_gz("rules_edge.json.gz")
        return [(rec, data["sets"][rec["set"]]["mask"]) for rec in data["positions"]]
    return [(rec, mask) for rec in load_gz("rules_%s.json.gz" % name) for mask in [BLOCK4_MASK if name == "block4" else 0]]


def test_edge_fixture_holds_the_families_it_was_written_for():
    data = load_gz("rules_edge.json.gz")
    recs = data["positions"]
    assert 1400 <= len(recs) <= 1600
    assert os.path.getsize(os.path.join(GOLDEN, "rules_edge.json.gz")) <= os.path.getsize(os.path.join(GOLDEN, "rules_noblock.json.gz"))
    assert data["sets"]["none"]["mask"] == 0 and data["sets"]["block4"]["mask"] == BLOCK4_MASK
    assert data["sets"]["block3"]["mask"] == BLOCK3_MASK
    wall = data["sets"]["wall8"]["mask"]
    assert bin(wall).count("1") >= 8 and not rr.legal_moves(rr.Board.from_masks(1, 1 << 48, wall, 0))  # a1 is walled in
    for name in data["sets"]:
        for fam in ("random", "few", "stuck", "full", "near", "wide", "capture"):
            sides = {r["to_move"] for r in recs if r["set"] == name and r["family"] == fam}
            assert sides == {1, 2}, (name, fam)
    n_moves = lambda r: 0 if r["moves"] == ["0000"] else len(r["moves"])
    wide = [n_moves(r) for r in recs if r["family"] == "wide"]
    assert sum(n > 128 for n in wide) >= 40 and sum(n > 170 for n in wide) >= 10 and max(wide) < rr.MAX_MOVES
    assert all(r["cells"].count(1) and r["cells"].count(2) for r in recs if r["family"] == "wide")
    few = [r for r in recs if r["family"] == "few"]
    assert all(1 <= r["cells"].count(v) <= 3 for r in few for v in (1, 2))
    lone = {(r["set"], r["cells"].index(1)) for r in few if r["cells"].count(1) == 1 and r["cells"].count(2) == 1}
    for name, s in data["sets"].items():
        assert sum(1 for n, _ in lone if n == name) == 49 - len(s["cells"])  # a single stone on every playable square
    for r in recs:
        empties = r["cells"].count(0) - len(data["sets"][r["set"]]["cells"])
        if r["family"] in ("stuck", "stuck_both"):
            assert r["moves"] == ["0000"] and empties > 0 and r["result"] in (1, 2)
        if r["family"] == "full":
            assert empties == 0 and r["moves"] == ["0000"]
        if r["family"] == "near":
            assert empties in (1, 2)
        assert len(r["succ"]) == len(r["moves"])  # every successor, the pass included
    ties = [r for r in recs if r["family"] == "full" and r["cells"].count(1) == r["cells"].count(2)]
    assert len(ties) >= 8 and all(r["set"] == "block3" and r["result"] == 1 for r in ties)  # an exact tie goes to x
    assert any(n_moves(r) > 128 and r["set"] != "none" for r in recs)
    # capture extremes: eight flips, a wipe-out, a clone with several sources
    flips, wiped, sources = 0, 0, 0
    for r in recs:
        if r["family"] != "capture":
            continue
        b = rr.Board.from_fen(r["fen"])
        me, other = rr.mover(b), rr.O if b.turn == 0 else rr.X
        for m in rr.legal_moves(b):
            after = rr.make_move(b, m)
            flips = max(flips, b.count(other) - after.count(other))
            wiped += after.count(other) == 0
            if (m & 0xFF) == (m >> 8):
                sources = max(sources, sum(b.cells[n] == me for n in rr.NEAR[m >> 8]))
    assert flips == 8 and wiped >= 4 and sources >= 4
    assert len(data["perft"]) == 16 and sum(p["pass_inside"] for p in data["perft"]) >= 4


@pytest.mark.parametrize("name", ["noblock", "block4", "edge"])
def test_restatement_equals_the_reference_written_fixtures(name):
    recs = fixture_records(name)
    assert len(recs) > 1000
    for rec, mask in recs:
        b = rr.Board.from_fen(rec["fen"], mask)
        assert b.fen() == rec["fen"] and b.turn == rec["to_move"] - 1
        assert b.masks()[2] == mask and b.reference_cells() == rec["cells"]
        moves = rr.legal_moves(b)
        assert (sorted(rr.move_string(m) for m in moves) or ["0000"]) == rec["moves"], rec["fen"]
        assert not rr.orders_disagree(b), rec["fen"]
        assert rr.result(b) == rec["result"], rec["fen"]
        if name == "edge":
            assert sorted(rec["succ"]) == rec["moves"]
        for mv, fen2 in rec["succ"].items():
            assert rr.make_move(b, rr.move_from_string(mv)).fen() == fen2, (rec["fen"], mv)


@pytest.mark.parametrize("name", ["noblock", "block4", "edge"])
def test_restatement_equals_the_c_oracle(name):
    for i, (rec, mask) in enumerate(fixture_records(name)):
        b = rr.Board.from_fen(rec["fen"], mask)
        p = orc.pos_from_fen(rec["fen"])
        p.blockers |= mask
        assert (int(p.pieces[0]), int(p.pieces[1]), int(p.blockers), p.turn) == b.masks() + (b.turn,)
        assert orc.fen(p) == b.fen()
        moves = rr.legal_moves(b)
        assert [int(m) for m in orc.movegen(p)] == moves, rec["fen"]  # the same moves in the same order
        assert orc.result(p) == rr.result(b)
        assert (orc.features(p) == rr.features(b)).all()
        assert [int(v) for v in orc.board_cells(p)] == b.reference_cells()
        assert [orc.move_string(m) for m in moves] == [rr.move_string(m) for m in moves]
        for m in moves[:: max(1, len(moves) // 8)]:
            q = orc_pos(b)
            orc.lib().orc_makemove(q, m & 0xFF, m >> 8)
            assert (int(q.pieces[0]), int(q.pieces[1]), q.turn) == rr.make_move(b, m).masks()[:2] + (1 - b.turn,)
        if i % 16 == 0:
            assert orc.perft(p, 2) == rr.perft(b, 2), rec["fen"]


def test_perft_of_the_restatement_the_oracle_and_the_reference_agree():
    data = load_gz("rules_edge.json.gz")
    for ent in data["perft"]:
        mask = data["sets"][ent["set"]]["mask"]
        b = rr.Board.from_fen(ent["fen"], mask)
        for d, n in ent["depth"].items():
            assert rr.perft(b, int(d)) == n == orc.perft(orc_pos(b), int(d)), (ent["fen"], d)
        assert rr.perft_has_pass(b, 3) == ent["pass_inside"]
    with open(os.path.join(GOLDEN, "perft.json")) as f:
        table = json.load(f)
    for key, mask in (("noblock", 0), ("block4", BLOCK4_MASK)):
        b = rr.Board.from_fen(table[key]["fen"], mask)
        for d in ("1", "2", "3"):
            assert rr.perft(b, int(d)) == table[key]["depth"][d]


def test_a_side_without_stones_loses_before_the_move_list_is_looked_at():
    """The kernels' order (the reference's C++ get_board_result), on the boards where the reference's Python result() says
    otherwise: the side to move is walled in, its opponent has no stones, and the side to move still wins."""
    for b, mask in pocket_boards():
        assert rr.orders_disagree(b) and not rr.legal_moves(b) and b.count(rr.EMPTY) > 0
        assert rr.result(b) == 1 + b.turn == orc.result(orc_pos(b))
        assert rr.kernel_count(b) == 0
        # the pass-first order would hand the empty squares, more than the pocket holds, to the side without stones
        assert b.count(rr.EMPTY) > b.count(rr.mover(b))
    # without a pocket the same kind of board is a full one, and both orders agree on it
    for mask in (0, BLOCK3_MASK):
        b = rr.Board([rr.BLOCK if (mask >> sq) & 1 else rr.X for sq in range(49)], 0)
        assert rr.orders_disagree(b) and rr.result(b) == 1 == orc.result(orc_pos(b))
    # no stones at all (the reference asserts): the kernels' first check decides, o "wins"
    assert rr.result(rr.Board([rr.EMPTY] * 49, 0)) == 2 == orc.result(orc_pos(rr.Board([rr.EMPTY] * 49, 0)))


def test_seeded_hill_climb_stays_below_the_move_list_width():
    """wave_movegen writes its moves into a 256-entry array (AZH_MAX_MOVES) without a bound of its own.  This search documents
    the headroom; it is NOT a proof: a seeded single-cell hill climb (x to move, every cell free, the opponent may even be
    left without a stone, which only frees squares) from 30 random boards.  The widest board it finds has 197 moves,
    `x2xx2/x2xx2/x2xx2/x2xx2/x2xx1x/x2xx2/x2xx2 x`; 400 restarts found nothing wider."""
    widest = rr.Board.from_fen("x2xx2/x2xx2/x2xx2/x2xx2/x2xx1x/x2xx2/x2xx2 x")
    assert rr.count_moves(widest) == 197
    assert rr.count_moves(rr.Board.from_fen("oxxxxxx/7/7/xxxxxxx/xxxxxxx/7/4x2 x")) == 193  # the widest with a stone a side
    found = [rr.hill_climb(seed, restarts=10) for seed in (1, 2, 3)]
    found += [rr.hill_climb(4, blockers=mask, restarts=4) for mask in (BLOCK4_MASK, BLOCK3_MASK)]
    best_n, best = max(found, key=lambda t: t[0])
    assert best_n == rr.count_moves(best) == len(set(rr.legal_moves(best)))
    assert 190 <= best_n <= 197 < rr.MAX_MOVES, "widest board found: %d moves, %s" % (best_n, best.fen())
    assert len(orc.movegen(orc_pos(best))) == best_n


def test_rules_oracle_under_sanitizers_on_the_edge_positions():
    """oracle/ataxx_rules_oracle.c as a stand-alone program built with -fsanitize=address,undefined (oracle/rules_edge_main.c:
    nothing loaded into Python is sanitized), on every edge position and the walled-in boards: no report, and the counts it
    prints are the restatement's."""
    import subprocess

    oracle_dir = os.path.dirname(os.path.abspath(orc.__file__))
    subprocess.check_call(["make", "-s", "-C", oracle_dir, "_build/rules_edge_asan"])
    items = [(rr.Board.from_fen(rec["fen"], mask), mask) for rec, mask in fixture_records("edge")] + pocket_boards()
    text = "".join("%d %s\n" % (mask, b.fen()) for b, mask in items)
    run = subprocess.run([os.path.join(oracle_dir, "_build", "rules_edge_asan")], input=text, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(items)
    for line, (b, _) in zip(lines, items):
        moves = rr.legal_moves(b)
        stones = sum(49 - c.count(rr.EMPTY) - c.count(rr.BLOCK) for c in (rr.make_move(b, m) for m in moves))
        assert [int(v) for v in line.split()] == [len(moves), rr.result(b), rr.perft(b, 2), stones], b.fen()
