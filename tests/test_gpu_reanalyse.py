"""Reanalysis of stored plies on the MI355X (azh_samples_read_plies, azh_engine_root_report_device, azh_samples_retarget,
training.reanalyse, train.py --reanalyse-fraction): stored plies read back as they were stored, root reports turned into policy
targets and values on the device bit for bit as the host restatement has them, refusals that change nothing, and the whole path
from real games to minibatches.

A SampleStore needs torch imported before the library is loaded (link.require_torch_runtime), so the checks
(tests/reanalyse_gpu_checks.py) run in one fresh process, once for the module, and each test below reads its check's verdict."""
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import link, model, training
from tests.fresh_process import passed, verdicts_of
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    return verdicts_of("tests.reanalyse_gpu_checks", str(tmp_path_factory.mktemp("reanalyse") / "verdicts.json"))


def test_read_plies_returns_what_was_stored(verdicts):
    passed(verdicts, "check_read_plies")


def test_synthetic_reports_become_the_restated_targets(verdicts):
    passed(verdicts, "check_synthetic_reports")


def test_refusals_change_nothing_and_later_games_append_behind(verdicts):
    passed(verdicts, "check_refusals")


def test_minibatch_parity_after_retarget(verdicts):
    passed(verdicts, "check_minibatch_parity")


def test_whole_path_against_an_engine_driven_by_existing_calls(verdicts):
    passed(verdicts, "check_whole_path")


def test_walls_one_engine_per_mask(verdicts):
    passed(verdicts, "check_walls")


def test_train_cli_reanalyses_before_the_first_step(tmp_path):
    with open(os.path.join(GOLDEN, "train_entries.json")) as f:
        entries = json.load(f) * 3           # 18 games: the first ten are the validation set
    games = str(tmp_path / "games.json")
    with open(games, "w") as f:
        for e in entries:
            f.write(json.dumps(e) + "\n")
    conv, bn = model.random_init(1, 128, seed=3)
    old, new = str(tmp_path / "model-001.npy"), str(tmp_path / "model-002.npy")
    model.save_model(old, conv, bn)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--steps", "2", "--minibatch-size", "16", "--games",
                          games, "--old-path", old, "--new-path", new, "--reanalyse-fraction", "0.5", "--reanalyse-visits", "8",
                          "--reanalyse-slots", "8"], cwd=ROOT, capture_output=True, timeout=600)
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    out = res.stdout.decode()
    # the plan's counts, from the lines alone: the trainer's shuffle, then the candidate plies of games [10, 18) that are no passes
    state = random.getstate()
    random.seed(123456789)
    shuffled = training.load_entries([games])
    random.setstate(state)
    arrays = link.entries_to_arrays(shuffled)
    c = 0
    for first, plies, word, _ in arrays.games[10:].tolist():
        f = arrays.ply_flags[first:first + plies]
        cand = (f & link.SAMPLES_PLY_FULL) != 0 if word & link.SAMPLES_GAME_HAS_FULL else np.ones(plies, dtype=bool)
        c += int((cand & ((f & link.SAMPLES_PLY_PASS) == 0)).sum())
    picked = round(0.5 * c)
    assert picked > 16 and "0 plies whose target does not sum to one" in out
    m = re.search(r"Reanalysis: (\d+) plies changed, (\d+) unchanged in (\d+) rounds of at most 8 slots at 8 visits", out)
    assert m, out[-2000:]
    assert int(m.group(1)) + int(m.group(2)) == picked and int(m.group(3)) == (picked + 7) // 8
    assert int(m.group(2)) == 0                                             # a finite net leaves no picked ply as it was
    assert out.index("Reanalysis:") < out.index("=== BEGINNING TRAINING ===") and "Step:    0 -- loss:" in out
    assert os.path.exists(new)
