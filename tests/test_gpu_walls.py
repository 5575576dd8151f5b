"""Walls through the loop on the MI355X: the store's gather and surprise pass with per-game wall masks
(tests/walls_gpu_checks.py, in one fresh process for the reason tests/test_gpu_samples.py gives), the generator's
--record-blockers / --start-fen, train.py on such lines, the UAI front-end and the ringmaster on walled boards.  Every move
is checked against tests/rules_reference.py on the walled board."""
import json
import os
import re
import subprocess
import sys

import pytest

from ataxxzero_amd import link, model, selfplay, uai
from tests import rules_reference as rr
from tests import walls_fixtures as wf
from tests.fresh_process import passed, verdicts_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSAL = "not its own image under all 8 symmetries"


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    return verdicts_of("tests.walls_gpu_checks", str(tmp_path_factory.mktemp("walls") / "verdicts.json"))


def test_gather_writes_the_walls_of_every_game(verdicts):
    passed(verdicts, "check_gather_with_walls")


def test_surprise_kernel_with_walls_equals_the_host(verdicts):
    passed(verdicts, "check_surprise_with_walls")


@pytest.fixture(scope="module")
def net_path(tmp_path_factory):
    conv, bn = model.random_init(2, 64, seed=3)
    path = str(tmp_path_factory.mktemp("net") / "net.npy")
    model.save_model(path, conv, bn)
    return path


# ---------------------------------------------------------------- the generator

def _generate(net_path, out, extra):
    cmd = [sys.executable, os.path.join(ROOT, "accelerated_generate_games.py"), "--network", net_path, "--output-games", out,
           "--game-count", "4", "--buffer-size", "2", "--visits", "8", "--seed", "1"] + extra
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, timeout=300)


def _lines(net_path, directory, name, extra):
    out = str(directory / name)
    res = _generate(net_path, out, extra)
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    with open(out, "rb") as f:
        return f.read().splitlines()


@pytest.fixture(scope="module")
def generated(net_path, tmp_path_factory):
    """{fen: (lines with the key, lines without)} for the default start and the asymmetric one."""
    directory = tmp_path_factory.mktemp("games")
    out = {}
    for tag, fen in (("default", None), ("asymmetric", wf.ASYMMETRIC_FEN)):
        start = [] if fen is None else ["--start-fen", fen]
        out[fen or wf.DEFAULT_FEN] = (_lines(net_path, directory, tag + "-keyed.json", start + ["--record-blockers"]),
                                      _lines(net_path, directory, tag + "-plain.json", start))
    return out


@pytest.mark.parametrize("fen,cells", [(wf.DEFAULT_FEN, [17, 23, 25, 31]), (wf.ASYMMETRIC_FEN, wf.ASYMMETRIC_CELLS)])
def test_generator_records_the_walls_it_plays_on(generated, fen, cells):
    keyed, plain = generated[fen]
    assert len(keyed) == len(plain) == 4
    key = b'"blockers":' + json.dumps(cells, separators=(",", ":")).encode() + b","
    for with_key, without in zip(keyed, plain):
        assert with_key == without[:1] + key + without[1:]            # the same games, the key's bytes apart
        entry = json.loads(with_key)
        assert entry["blockers"] == cells and list(entry)[0] == "blockers"
        board = rr.Board.from_fen(fen)
        for ply, text in enumerate(entry["moves"]):
            assert entry["boards"][ply] == board.reference_cells()
            legal = {rr.move_string(m) for m in rr.legal_moves(board)}
            assert text in legal, (ply, text)
            assert entry["dists"][ply] and set(entry["dists"][ply]) <= legal, (ply, set(entry["dists"][ply]) - legal)
            board = rr.make_move(board, rr.move_from_string(text))


def test_generator_refuses_the_random_symmetry_on_asymmetric_walls(net_path, tmp_path):
    out = str(tmp_path / "games.json")
    res = _generate(net_path, out, ["--start-fen", wf.ASYMMETRIC_FEN, "--random-symmetry"])
    assert res.returncode != 0 and REFUSAL in res.stderr.decode() and "Traceback" not in res.stderr.decode()
    assert "0x%x" % selfplay.parse_fen(wf.ASYMMETRIC_FEN)[2] in res.stderr.decode()
    assert not os.path.exists(out) or os.path.getsize(out) == 0
    # with the symmetric default walls the mode runs
    res = _generate(net_path, out, ["--random-symmetry", "--record-blockers"])
    assert res.returncode == 0, res.stderr.decode()[-3000:]


# ---------------------------------------------------------------- the trainer

def _train(net_path, tmp_path, lines, extra):
    games = str(tmp_path / "games.json")
    with open(games, "wb") as f:
        f.write(b"\n".join(lines) + b"\n")
    new = str(tmp_path / "model-002.npy")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--steps", "3", "--minibatch-size", "16", "--games", games,
           "--old-path", net_path, "--new-path", new] + extra
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, timeout=600)
    assert res.returncode == 0 and os.path.exists(new), res.stderr.decode()[-3000:]
    return res.stdout.decode()


def _training_lines(generated, keyed):
    which = 0 if keyed else 1
    return generated[wf.DEFAULT_FEN][which] + generated[wf.ASYMMETRIC_FEN][which] + generated[wf.DEFAULT_FEN][which]


def test_train_cli_with_device_samples_on_walled_games(generated, net_path, tmp_path):
    out = _train(net_path, tmp_path, _training_lines(generated, True), ["--device-samples"])
    line = next(l for l in out.splitlines() if l.startswith("Device samples:"))
    assert "Device samples: 12 games" in line and line.endswith("; 12 games on 2 wall maps.")
    assert "Step:    0 -- loss:" in out


def test_train_cli_with_surprise_weight_on_walled_games(generated, net_path, tmp_path):
    out = _train(net_path, tmp_path, _training_lines(generated, True), ["--surprise-weight", "0.5", "--surprise-dtype", "f32"])
    assert "; 12 games on 2 wall maps." in out
    masked = next(l for l in out.splitlines() if l.startswith("Policy surprise:"))
    assert masked.rstrip().endswith(" 0 targets that are no legal moves.")
    # the same games without the key: the pass the trainer made before — the prior's softmax runs over the wall cells
    (tmp_path / "bare").mkdir()
    out = _train(net_path, tmp_path / "bare", _training_lines(generated, False), ["--surprise-weight", "0.5", "--surprise-dtype", "f32"])
    assert "wall maps" not in out
    bare = next(l for l in out.splitlines() if l.startswith("Policy surprise:"))
    pattern = r"KL mean ([0-9.]+), median ([0-9.]+), max ([0-9.]+)"
    print(masked, bare, sep="\n")
    assert re.search(pattern, masked).groups() != re.search(pattern, bare).groups()


# ---------------------------------------------------------------- the UAI front-end

def _go(session):
    out, more = session.handle("go movetime 1000")
    assert more and out[-1].startswith("bestmove ")
    return out, out[-1].split()[1]


@pytest.mark.parametrize("options", [{}, {"parallel_leaves": 4}, {"solver": True}, {"reuse_tree": True}],
                         ids=["plain", "parallel-leaves", "solver", "reuse-tree"])
@pytest.mark.parametrize("fen", [wf.DEFAULT_FEN, wf.ASYMMETRIC_FEN], ids=["default", "asymmetric"])
def test_uai_session_plays_on_the_walled_board(net_path, options, fen):
    searcher = uai.Searcher(net_path, dtype="f16", **options)
    session = uai.Session(searcher, visits=16)
    session.handle("uainewgame")
    session.handle("position fen " + fen)
    assert session.position.blockers == selfplay.parse_fen(fen)[2]
    board = rr.Board.from_fen(fen)
    for ply in range(12):
        _, text = _go(session)
        assert wf.is_legal_text(board, text), (ply, text, board.fen())
        board = rr.make_move(board, rr.move_from_string(text))
        session.handle("moves " + text)
        assert session.position.fen() == board.fen()
    searcher.close()


def test_uai_session_passes_where_the_walls_leave_no_move(net_path):
    fen = "ooooooo/ooooooo/ooooooo/ooooooo/ooooooo/ooooooo/x--oooo x"     # a1's clone and jump squares are walls
    assert rr.legal_moves(rr.Board.from_fen(fen)) == [] and len(rr.legal_moves(rr.Board.from_fen(fen.replace("-", "1")))) == 2
    for options in ({}, {"parallel_leaves": 4}, {"solver": True}, {"reuse_tree": True}):
        searcher = uai.Searcher(net_path, dtype="f16", **options)
        session = uai.Session(searcher, visits=16)
        session.handle("position fen " + fen)
        walled = _go(session)[1]
        session.handle("position fen ooooooo/ooooooo/ooooooo/ooooooo/ooooooo/ooooooo/xoooooo x")      # a pass position today
        assert walled == _go(session)[1] == "0000"
        searcher.close()


def _inherited(lines):
    words = next(l for l in lines if l.startswith("info nodes ")).split()
    return int(words[words.index("inherited") + 1])


def test_uai_reuse_tree_starts_afresh_when_the_walls_change(net_path):
    searcher = uai.Searcher(net_path, dtype="f16", reuse_tree=True, show_pv=True)
    session = uai.Session(searcher, visits=16)
    session.handle("position fen " + wf.DEFAULT_FEN)
    _go(session)
    session.handle("position fen " + wf.DEFAULT_FEN)
    out, _ = _go(session)
    assert searcher.last_inherited == 16 and _inherited(out) == 16
    session.handle("position fen " + wf.DEFAULT_FEN.replace("3-3/2-1-2/3-3", "3-3/7/3-3"))       # the same stones, two walls fewer
    out, text = _go(session)
    assert searcher.last_inherited == 0 and _inherited(out) == 0
    assert wf.is_legal_text(rr.Board.from_fen("x5o/7/3-3/7/3-3/7/o5x x"), text)
    searcher.close()


@pytest.mark.parametrize("options", [{}, {"reuse_tree": True}], ids=["plain", "reuse-tree"])
def test_uai_random_symmetry_on_asymmetric_walls_says_so_and_searches(net_path, options):
    searcher = uai.Searcher(net_path, dtype="f16", random_symmetry=True, **options)
    session = uai.Session(searcher, visits=16)
    session.handle("position fen " + wf.ASYMMETRIC_FEN)
    for _ in range(2):
        out, text = _go(session)
        assert any(l.startswith("info string ") and REFUSAL in l for l in out), out
        assert wf.is_legal_text(rr.Board.from_fen(wf.ASYMMETRIC_FEN), text)
    session.handle("position fen " + wf.DEFAULT_FEN)                  # symmetric walls: the mode is on, nothing to say
    out, text = _go(session)
    assert not any(REFUSAL in l for l in out) and wf.is_legal_text(rr.Board.from_fen(wf.DEFAULT_FEN), text)
    searcher.close()


# ---------------------------------------------------------------- the ringmaster

def test_ringmaster_plays_its_match_on_the_walled_board(net_path, tmp_path):
    pgn = str(tmp_path / "games.pgn")
    engine = "python uai_interface.py --network-path %s --visits 8" % net_path
    cmd = [sys.executable, os.path.join(ROOT, "uai_ringmaster.py"), "--engine", engine, "--engine", engine, "--game-count", "4",
           "--opening-depth", "2", "--start-fen", wf.DEFAULT_FEN, "--pgn-out", pgn, "--seed", "5"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    with open(pgn) as f:
        blocks = f.read().split("\n\n")
    games = [b.split() for b in blocks if b.strip() and not b.lstrip().startswith("[")]
    assert len(games) == 4
    for moves in games:
        assert len(moves) > 2 and wf.replay_legal(wf.DEFAULT_FEN, moves) is None, moves
    walls = {"d5", "c4", "e4", "d3"}
    assert not any(m[-2:] in walls for moves in games for m in moves)
