"""The optimisation step on the MI355X (training.make_optimizer / train_step on the ROCm backend's kernels, and
training.train(device_draws=True) through the device sample store) against the float64 restatement of tests/step_reference.py.

train(device_draws=True) enqueues on torch's streams, so the process must hold ONE HIP runtime: torch imported before the
library is loaded (link.require_torch_runtime).  The checks (tests/step_gpu_checks.py) therefore run in one fresh process, once
for the module, and each test below reads its check's verdict."""
import json

import pytest

from tests import fresh_process

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    return fresh_process.verdicts_of("tests.step_gpu_checks", str(tmp_path_factory.mktemp("step") / "verdicts.json"))


def _passed(verdicts, name):
    print(json.dumps(verdicts["measured"].get(name)))
    fresh_process.passed(verdicts, name)


def test_step_on_device(verdicts):
    _passed(verdicts, "check_step_on_device")


def test_train_through_the_store(verdicts):
    _passed(verdicts, "check_train_through_the_store")


def test_device_equals_cpu_to_rounding(verdicts):
    _passed(verdicts, "check_device_equals_cpu_to_rounding")
