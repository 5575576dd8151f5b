"""The auxiliary training targets on the MI355X (include/ataxxzero_hip.h, "Auxiliary targets"; azh_samples_gather,
link.SampleStore.gather(aux=True), train.py --aux-*): ownership, score, reply and weights bit for bit those of the host
restatement (tests/aux_reference.py), from game lines and from ring records, with host draws and with draws made on the device,
and the three existing outputs byte for byte what the kernels without them write.

The checks (tests/aux_gpu_checks.py) run in one fresh process, once for the module, for the reason tests/test_gpu_samples.py
gives; each test below reads its check's verdict."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import model, training
from tests.fresh_process import passed, verdicts_of
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    return verdicts_of("tests.aux_gpu_checks", str(tmp_path_factory.mktemp("aux") / "verdicts.json"))


def test_parity_from_game_lines(verdicts):
    passed(verdicts, "check_parity_from_game_lines")


def test_parity_from_records(verdicts):
    passed(verdicts, "check_parity_from_records")


def test_parity_of_the_existing_outputs(verdicts):
    passed(verdicts, "check_parity_of_the_existing_outputs")


def test_edges_of_the_wave_for_the_reply_scatter(verdicts):
    passed(verdicts, "check_edges_of_the_wave_for_the_reply_scatter")


def test_reply_absent(verdicts):
    passed(verdicts, "check_reply_absent")


def test_device_draws_with_aux(verdicts):
    passed(verdicts, "check_device_draws_with_aux")


def test_stale_rows(verdicts):
    passed(verdicts, "check_stale_rows")


def test_no_owners_anywhere(verdicts):
    passed(verdicts, "check_no_owners_anywhere")


def test_ingest_refusals(verdicts):
    passed(verdicts, "check_ingest_refusals")


@pytest.mark.parametrize("flags", [["--device-samples"], ["--device-draws"]])
def test_train_cli_with_aux_targets(tmp_path, flags):
    with open(os.path.join(GOLDEN, "train_entries.json")) as f:
        entries = json.load(f) * 3           # 18 games: the first ten are the validation set
    games = str(tmp_path / "games.json")
    with open(games, "w") as f:
        for e in entries:
            f.write(json.dumps(e) + "\n")
    conv, bn = model.random_init(1, 128, seed=3)
    old, new = str(tmp_path / "model-001.npy"), str(tmp_path / "model-002.npy")
    model.save_model(old, conv, bn)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--steps", "3", "--minibatch-size", "16", "--games",
                          games, "--old-path", old, "--new-path", new, "--aux-ownership", "1.5", "--aux-score", "0.5",
                          "--aux-reply", "0.15"] + flags, cwd=ROOT, capture_output=True, timeout=600)
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    out = res.stdout.decode()
    assert "Auxiliary targets: 8 of 8 training games have owners" in out
    step0 = next(line for line in out.splitlines() if line.startswith("Step:    0 -- loss:"))
    assert " own: " in step0 and " score: " in step0 and " reply: " in step0 and step0.endswith(")")
    conv2, _ = model.load_model(new)
    assert [a.shape for a in conv2] == [a.shape for a in conv]
    assert any(not np.array_equal(a, b) for a, b in zip(conv, conv2))       # weights moved
    fresh = training.aux_random_init(128, training.AUX_SEED)
    with np.load(training.aux_sidecar(new), allow_pickle=False) as kept:
        assert sorted(kept.files) == sorted(fresh)
        assert all(kept[k].shape == fresh[k].shape and not np.array_equal(kept[k], fresh[k]) for k in fresh)
