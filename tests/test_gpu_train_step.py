"""The optimisation step on the MI355X (training.make_optimizer / train_step on the ROCm backend's kernels, and
training.train(device_draws=True) through the device sample store) against the float64 restatement of tests/step_reference.py.

train(device_draws=True) enqueues on torch's streams, so the process must hold ONE HIP runtime: torch imported before the
library is loaded (link.require_torch_runtime).  The checks (tests/step_gpu_checks.py) therefore run in one fresh process, once
for the module, and each test below reads its check's verdict."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("step") / "verdicts.json")
    res = subprocess.run([sys.executable, "-m", "tests.step_gpu_checks", path], cwd=ROOT, capture_output=True, timeout=600)
    assert res.returncode == 0 and os.path.exists(path), (res.stdout.decode()[-2000:], res.stderr.decode()[-4000:])
    with open(path) as f:
        return json.load(f)


def _passed(verdicts, name):
    assert name in verdicts, "not run: an earlier check ended in a device error (%s)" % ", ".join(verdicts)
    print(json.dumps(verdicts["measured"].get(name)))
    assert verdicts[name] == "ok", "\n" + verdicts[name]


def test_step_on_device(verdicts):
    _passed(verdicts, "check_step_on_device")


def test_train_through_the_store(verdicts):
    _passed(verdicts, "check_train_through_the_store")


def test_device_equals_cpu_to_rounding(verdicts):
    _passed(verdicts, "check_device_equals_cpu_to_rounding")
