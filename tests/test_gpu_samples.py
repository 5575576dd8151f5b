"""The device-resident sample store on the MI355X (azh_samples_*, link.SampleStore, training.make_minibatch_device,
train.py --device-samples): minibatches bit for bit those of the host pipeline, from game lines and from ring records, with
host draws and with draws made on the device.

A SampleStore enqueues on torch's streams and writes torch's tensors, so the process must hold ONE HIP runtime: torch
imported before the library is loaded (link.require_torch_runtime).  A pytest process that has run other device tests loaded
the library first, so the checks (tests/samples_gpu_checks.py) run in one fresh process, once for the module, and each test
below reads its check's verdict (tests/fresh_process.py)."""
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
    return verdicts_of("tests.samples_gpu_checks", str(tmp_path_factory.mktemp("samples") / "verdicts.json"))


def test_reference_parity(verdicts):
    passed(verdicts, "check_reference_parity")


def test_every_index_under_every_symmetry(verdicts):
    passed(verdicts, "check_every_index_under_every_symmetry")


def test_edges_of_the_wave(verdicts):
    passed(verdicts, "check_edges_of_the_wave")


def test_the_record_path(verdicts):
    passed(verdicts, "check_the_record_path")


def test_device_draws(verdicts):
    passed(verdicts, "check_device_draws")


def test_stream_and_reuse(verdicts):
    passed(verdicts, "check_stream_and_reuse")


def test_capacity(verdicts):
    passed(verdicts, "check_capacity")


def test_bad_ply(verdicts):
    passed(verdicts, "check_bad_ply")


def test_argument_refusals(verdicts):
    passed(verdicts, "check_argument_refusals")


@pytest.mark.parametrize("flags", [["--device-samples"], ["--device-draws"]])
def test_train_cli_with_device_samples(tmp_path, flags):
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
                          games, "--old-path", old, "--new-path", new] + flags, cwd=ROOT, capture_output=True, timeout=600)
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    out = res.stdout.decode()
    assert "Found %d games" % len(entries) in out and "Step:    0 -- loss:" in out and "Device samples: %d games" % len(entries) in out
    conv2, bn2 = model.load_model(new)
    assert [a.shape for a in conv2] == [a.shape for a in conv]
    assert any(not np.array_equal(a, b) for a, b in zip(conv, conv2))       # weights moved
