"""The start pool's host side: the uid rule, the FEN-file parser and the command lines' refusals — all reached without a device —
and the maps the GPU tests play on (tests/start_pool_fixtures.py)."""
import os
import subprocess
import sys

import pytest

from ataxxzero_amd import link, selfplay
from tests import start_pool_fixtures as spf
from tests import walls_fixtures as wf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_of_a_uid_is_round_robin_over_strides():
    for n in (1, 2, 3, 4, 7, 64):
        for stride in (1, 2, 3):
            for uid in list(range(0, 200)) + [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]:
                assert link.start_pool_entry(uid, n, stride) == (uid // stride) % n, (uid, n, stride)
    # every prefix of a uid-ordered file is balanced over the maps: no map is ever more than one game ahead
    counts = [0, 0, 0]
    for uid in range(100):
        counts[link.start_pool_entry(uid, 3, 1)] += 1
        assert max(counts) - min(counts) <= 1
    # a two-net match: slots 2k and 2k + 1 share a map
    assert all(link.start_pool_entry(2 * k, 5, 2) == link.start_pool_entry(2 * k + 1, 5, 2) == k % 5 for k in range(40))
    for n, stride in ((0, 1), (-1, 1), (3, 0)):
        with pytest.raises(link.AzhError):
            link.start_pool_entry(5, n, stride)


def test_the_fen_file_parser(tmp_path):
    path = tmp_path / "maps.txt"
    path.write_text("# three maps\n\n%s\n   \n  %s  \n# the asymmetric one\n%s\n" % (wf.PLAIN_FEN, wf.DEFAULT_FEN, wf.ASYMMETRIC_FEN))
    assert selfplay.parse_fen_file(str(path)) == [wf.PLAIN_FEN, wf.DEFAULT_FEN, wf.ASYMMETRIC_FEN]


@pytest.mark.parametrize("text,why", [
    ("# nothing\n\n", "holds no position"),
    (wf.PLAIN_FEN + "\nx5o/7/7/7/7/7/o5q x\n", "line 2: bad FEN"),
    ("x6/7/7/7/7/7/7 x\n", "line 1: a side has no stone"),
    ("\nxo-----/-------/-------/7/7/7/7 x\n", "line 2: the position is finished"),
    ("x6o/7/7/7/7/7/o5x x\n", "line 1: a row is longer than 7 cells"),
])
def test_the_fen_file_parser_names_the_file_and_the_line(tmp_path, text, why):
    path = tmp_path / "maps.txt"
    path.write_text(text)
    with pytest.raises(ValueError) as err:
        selfplay.parse_fen_file(str(path))
    assert why in str(err.value) and "maps.txt" in str(err.value)


def test_start_refusal_agrees_with_the_oracle_on_the_test_maps():
    for entry in spf.entries():
        assert selfplay.start_refusal(*entry) is None
        assert selfplay.parse_fen(spf.fen_of(entry)) == entry
    x, o, walls, turn = spf.entries()[3]
    full = spf.BOARD & ~(x | o)
    assert "finished" in selfplay.start_refusal(x, o, full, turn)          # every empty cell a wall: nobody can move
    assert "wall" in selfplay.start_refusal(x, o, walls | (x & -x), turn)


def _run(script, *flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + list(flags), cwd=ROOT, capture_output=True, text=True,
                          timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))


def test_the_generator_refuses_before_a_device_is_opened(tmp_path):
    maps = tmp_path / "maps.txt"
    maps.write_text(wf.DEFAULT_FEN + "\n" + wf.ASYMMETRIC_FEN + "\n")
    base = ["--network", str(tmp_path / "none.npy"), "--output-games", str(tmp_path / "out-0.json"), "--visits", "4"]
    res = _run("accelerated_generate_games.py", *base, "--start-fens", str(maps), "--start-fen", wf.PLAIN_FEN)
    assert res.returncode != 0 and "--start-fens and --start-fen exclude each other" in res.stderr
    res = _run("accelerated_generate_games.py", *base, "--start-fens", str(maps), "--random-symmetry")
    mask = selfplay.parse_fen(wf.ASYMMETRIC_FEN)[2]
    assert res.returncode != 0 and "--random-symmetry: " + selfplay.symmetry_refusal(mask) in res.stderr
    res = _run("accelerated_generate_games.py", *base, "--start-fens", str(tmp_path / "missing.txt"))
    assert res.returncode != 0 and "--start-fens:" in res.stderr
    maps.write_text("x6/7/7/7/7/7/7 x\n")
    res = _run("accelerated_generate_games.py", *base, "--start-fens", str(maps))
    assert res.returncode != 0 and "line 1: a side has no stone" in res.stderr
    assert not os.path.exists(str(tmp_path / "out-0.json"))
