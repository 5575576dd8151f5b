"""Lambda-returns as value targets on the MI355X (azh_samples_value_returns, train.py --value-lambda): the kernel's returns are
the restatement's bit for bit, at the chunk edges of its 64-lane walk, with and without proofs; the four minibatch kernels write
them as the value and nothing else moves; lambda 1 and 0 are z and the blend of 1.0; clearing, a second pass, a sub-range and
refusals behave as the header says; and the host pipeline gives the same value column for the same draws.

A SampleStore needs torch imported before the library is loaded (link.require_torch_runtime), so the checks
(tests/value_lambda_gpu_checks.py) run in one fresh process, once for the module, and each test below reads its check's verdict."""
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import training
from tests.fresh_process import passed, verdicts_of
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    return verdicts_of("tests.value_lambda_gpu_checks", str(tmp_path_factory.mktemp("value_lambda") / "verdicts.json"))


def test_returns_are_the_restatement_bit_for_bit(verdicts):
    passed(verdicts, "check_returns_are_the_restatement")


def test_returns_with_proofs(verdicts):
    passed(verdicts, "check_returns_with_proofs")


def test_minibatches_write_the_returns_and_nothing_else_moves(verdicts):
    passed(verdicts, "check_minibatches_write_the_returns")


def test_lambda_one_is_z_and_lambda_zero_the_blend_of_one(verdicts):
    passed(verdicts, "check_lambda_one_and_zero")


def test_clear_restores_every_byte(verdicts):
    passed(verdicts, "check_clear_restores_every_byte")


def test_second_pass_replaces_and_sub_range_leaves_the_rest(verdicts):
    passed(verdicts, "check_second_pass_and_sub_range")


def test_refusals_change_nothing(verdicts):
    passed(verdicts, "check_refusals_change_nothing")


def test_host_and_device_pipelines_agree(verdicts):
    passed(verdicts, "check_host_and_device_pipelines_agree")


def test_train_cli_computes_the_returns_after_the_proofs(tmp_path):
    with open(os.path.join(GOLDEN, "train_entries.json")) as f:
        entries = json.load(f) * 3           # 18 games: the first ten are the validation set
    rng = np.random.default_rng(3)
    for e in entries[::2]:
        e["values"] = rng.uniform(-1.0, 1.0, len(e["boards"])).tolist()
    games = str(tmp_path / "games.json")
    with open(games, "w") as f:
        for e in entries:
            f.write(json.dumps(e) + "\n")
    new = str(tmp_path / "model-002.npy")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--steps", "2", "--minibatch-size", "16", "--games",
                          games, "--new-path", new, "--prove-depth", "2", "--value-lambda", "0.7"], cwd=ROOT,
                         capture_output=True, timeout=600)
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    out = res.stdout.decode()
    state = random.getstate()
    random.seed(123456789)
    shuffled = training.load_entries([games])[10:]           # the trainer's shuffle: the training games
    random.setstate(state)
    valued = [e for e in shuffled if "values" in e]
    m = re.search(r"Value targets: lambda-returns \(L = 0\.7\) over (\d+) plies of (\d+) games; (\d+) games without values "
                  r"keep z\.", out)
    assert m, out[-2000:]
    assert [int(v) for v in m.groups()] == [sum(len(e["boards"]) for e in valued), len(valued), len(shuffled) - len(valued)]
    assert 0 < len(valued) < len(shuffled)
    assert out.index("Proofs:") < out.index("Value targets:") < out.index("=== BEGINNING TRAINING ===")
    assert "Step:    0 -- loss:" in out and os.path.exists(new)
