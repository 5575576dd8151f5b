"""Policy surprise weighting on the MI355X (azh_samples_surprise*, azh_samples_set_ply_weights, link.SampleStore.surprise,
train.py --surprise-weight): the surprise kernel bit for bit against its host restatement, the tower-fed pass against the
float64 oracle, the weighted draws against theirs.

The checks (tests/surprise_gpu_checks.py) run in one fresh process, once for the module, for the reason tests/test_gpu_samples.py
gives; each test below reads its check's verdict."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import model
from tests.fresh_process import passed, verdicts_of
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    return verdicts_of("tests.surprise_gpu_checks", str(tmp_path_factory.mktemp("surprise") / "verdicts.json"), echo=True)


def test_surprise_from_logits_equals_the_host_bit_for_bit(verdicts):
    passed(verdicts, "check_from_logits_bit_exact")


def test_surprise_of_a_net_against_the_float64_oracle(verdicts):
    passed(verdicts, "check_net_surprise")


def test_weighted_draws_and_ply_weights(verdicts):
    passed(verdicts, "check_weighted_draws")


def _train(tmp_path, extra, with_old=True):
    with open(os.path.join(GOLDEN, "train_entries.json")) as f:
        entries = json.load(f) * 3           # 18 short games: the first ten are the validation set
    games = str(tmp_path / "games.json")
    with open(games, "w") as f:
        for e in entries:
            f.write(json.dumps(e) + "\n")
    conv, bn = model.random_init(1, 128, seed=3)
    old, new = str(tmp_path / "model-001.npy"), str(tmp_path / "model-002.npy")
    model.save_model(old, conv, bn)
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--steps", "3", "--minibatch-size", "16", "--games", games,
           "--new-path", new] + (["--old-path", old] if with_old else []) + extra
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, timeout=600), len(entries), conv, new


def test_train_cli_with_surprise_weight(tmp_path):
    res, n, conv, new = _train(tmp_path, ["--surprise-weight", "0.5"])
    assert res.returncode == 0, res.stderr.decode()[-3000:]      # (train() raises when store.status() is not 0 at the end)
    out = res.stdout.decode()
    assert "Device samples: %d games" % n in out and "Step:    0 -- loss:" in out
    line = next(l for l in out.splitlines() if l.startswith("Policy surprise:"))
    assert "%d games" % (n - 10) in line and "KL mean" in line and "median" in line and "max" in line and "share" in line
    assert line.rstrip().endswith(" 0 targets that are no legal moves.")
    conv2, _ = model.load_model(new)
    assert any(not np.array_equal(a, b) for a, b in zip(conv, conv2))       # weights moved


def test_train_cli_refuses_surprise_weight_without_old_path(tmp_path):
    res, _, _, new = _train(tmp_path, ["--surprise-weight", "0.5"], with_old=False)
    assert res.returncode != 0 and not os.path.exists(new)
    err = res.stderr.decode()
    assert "--surprise-weight" in err and "--old-path" in err and "Traceback" not in err
