"""Proven outcomes for stored plies on the MI355X (azh_samples_prove, azh_samples_proofs, train.py --prove-depth): the proofs
are the alpha-beta search's, on plain games and on walled roots under budgets; minibatches change in the proven plies' value
entries and nowhere else; proofs only accumulate; refusals change nothing; and the trainer reports what a recount finds.

A SampleStore needs torch imported before the library is loaded (link.require_torch_runtime), so the checks
(tests/prove_gpu_checks.py) run in one fresh process, once for the module, and each test below reads its check's verdict."""
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import link, training
from tests.fresh_process import passed, verdicts_of
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    return verdicts_of("tests.prove_gpu_checks", str(tmp_path_factory.mktemp("prove") / "verdicts.json"))


def test_proofs_are_the_searchs(verdicts):
    passed(verdicts, "check_proofs_are_the_searchs")


def test_deep_rows_walls_and_budgets(verdicts):
    passed(verdicts, "check_deep_rows_walls_budgets")


def test_minibatches_change_in_proven_value_entries_only(verdicts):
    passed(verdicts, "check_minibatches")


def test_proofs_only_accumulate(verdicts):
    passed(verdicts, "check_monotone")


def test_refusals_change_nothing(verdicts):
    passed(verdicts, "check_refusals")


def test_train_cli_proves_before_the_first_step(tmp_path):
    with open(os.path.join(GOLDEN, "train_entries.json")) as f:
        entries = json.load(f) * 3           # 18 games: the first ten are the validation set
    games = str(tmp_path / "games.json")
    with open(games, "w") as f:
        for e in entries:
            f.write(json.dumps(e) + "\n")
    new = str(tmp_path / "model-002.npy")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--steps", "2", "--minibatch-size", "16", "--games",
                          games, "--new-path", new, "--prove-depth", "3", "--prove-policy"], cwd=ROOT, capture_output=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    out = res.stdout.decode()
    # the recount: the trainer's shuffle, then every ply of games [10, 18) (no pass, no "full") searched by existing calls
    state = random.getstate()
    random.seed(123456789)
    shuffled = training.load_entries([games])
    random.setstate(state)
    arrays = link.entries_to_arrays(shuffled)
    first = int(arrays.games[10][0])
    assert not arrays.ply_flags.any() and "0 plies whose target does not sum to one" in out
    boards = arrays.boards[first:].copy()
    ply = np.concatenate([np.arange(n) for _, n, _, _ in arrays.games[10:].tolist()])
    result = np.concatenate([np.full(n, word & 0xFF) for _, n, word, _ in arrays.games[10:].tolist()])
    boards[:, 0] |= (ply.astype(np.uint64) & np.uint64(1)) << np.uint64(63)
    found = link.alphabeta_search(boards, 0, 3)
    proven = np.abs(found.values) >= link.ALPHABETA_WIN
    wins, losses = proven & (found.values > 0), proven & (found.values < 0)
    against = proven & ((found.values > 0) != (result == 1 + (ply & 1)))
    m = re.search(r"Proofs: (\d+) proven wins, (\d+) proven losses among (\d+) plies searched to depth 3 \(no node limit\); "
                  r"(\d+) contradict their game's result; (\d+) policy targets replaced", out)
    assert m, out[-2000:]
    assert [int(v) for v in m.groups()] == [int(wins.sum()), int(losses.sum()), len(boards), int(against.sum()),
                                            int((wins & (found.moves != 0xFFFF)).sum())]
    assert int(wins.sum()) > 20 and int(losses.sum()) > 0 and int(against.sum()) > 0
    assert out.index("Proofs:") < out.index("=== BEGINNING TRAINING ===") and "Step:    0 -- loss:" in out
    assert os.path.exists(new)
