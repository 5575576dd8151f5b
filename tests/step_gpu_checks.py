"""The device checks of tests/test_gpu_train_step.py, run in a process of their own: train(device_draws=True) has a SampleStore
write torch's tensors on torch's streams, so torch must be imported before the library is loaded (link.require_torch_runtime).
`python -m tests.step_gpu_checks OUT.json` runs every check once and writes {name: "ok" | traceback, "measured": {name: the
distances it saw}}; after a check that ends in a device error nothing more is run.

On the GPU the step runs on the ROCm backend's convolutions and batch norm, kernels this project did not write: here their
conventions (moving variance, eps, momentum) are held to the float64 restatement (tests/step_reference.py), and so is the
seam between the HIP minibatch kernel's seven outputs and the loss.  The allowance is 8 x d32 per quantity (d32:
tests/test_train_step_host.py) — twice the CPU's factor, for atomics and algorithm choice in the backend's reductions — under the
same condition: below a quarter of what separates the two moving-variance rules."""
import os
import tempfile

import numpy as np
import torch

from ataxxzero_amd import training
from tests import fresh_process
from tests import step_reference as ref
from tests import test_train_step_host as host

FACTOR = 8
SYNTHETIC_SEED = 158              # minibatches and a start net that keep the ReLU inputs off the kink (host.KINK_FACTOR)
STORE_NET_SEED = 36
MEASURED = {}
THROUGH_THE_STORE = {}            # check_train_through_the_store's start, minibatches and result, for the check after it


def check_step_on_device():
    start = host.start_net(2, 32, 11, aux=True)
    start["bn"] = host.settled(start["conv"], ref.synthetic_batch(np.random.default_rng(6), 64))
    batches = host.synthetic_batches(SYNTHETIC_SEED, 16, True)
    want, d32, allowed, gap = host.float32_allowance(start, batches, host.AUX_LOSS_WEIGHTS, FACTOR)
    got = host.trainer_steps(start, batches, host.AUX_LOSS_WEIGHTS, torch.float32, "cuda")
    MEASURED["check_step_on_device"] = {"d32": d32, "gap": gap, "distance": ref.distances(got, want, start)}
    host.check_within(got, want, start, allowed)


def check_train_through_the_store():
    with tempfile.TemporaryDirectory() as directory:
        games, old, start = host.fixture_games(directory, STORE_NET_SEED)
        start["aux"] = training.aux_random_init(32, training.AUX_SEED)
        new = os.path.join(directory, "new.npy")
        keeper = host.KeptBatches(training.make_minibatch_device, 3)
        training.make_minibatch_device = keeper
        try:
            training.train([games], old, new, steps=3, minibatch_size=16, learning_rate=host.LR, device=torch.device("cuda"),
                           log=lambda line: None, device_draws=True,
                           **dict(zip(("aux_ownership", "aux_score", "aux_reply"), host.AUX_LOSS_WEIGHTS)))
        finally:
            training.make_minibatch_device = keeper.make
        got = host.saved(new, True)
    batches = keeper.kept
    assert len(batches) == 3 and all(len(b) == 7 and len(b[0]) == 16 for b in batches)
    assert batches[0][0].tobytes() != batches[1][0].tobytes() != batches[2][0].tobytes()     # copies, not one reused tensor
    assert all(np.abs(b[4]).max() > 1 for b in batches)                                      # the score arrives in stones
    want, d32, allowed, gap = host.float32_allowance(start, batches, host.AUX_LOSS_WEIGHTS, FACTOR)
    MEASURED["check_train_through_the_store"] = {"d32": d32, "gap": gap, "distance": ref.distances(got, want, start)}
    THROUGH_THE_STORE.update(start=start, batches=batches, got=got)
    host.check_within(got, want, start, allowed)


def check_device_equals_cpu_to_rounding():
    """Reported, not asserted: which side moved, should either check above ever fail."""
    assert THROUGH_THE_STORE, "check_train_through_the_store kept no minibatches"
    start, batches, got = (THROUGH_THE_STORE[k] for k in ("start", "batches", "got"))
    cpu = host.trainer_steps(start, batches, host.AUX_LOSS_WEIGHTS, torch.float32, "cpu")
    cpu["losses"] = None
    MEASURED["check_device_equals_cpu_to_rounding"] = {"distance": ref.distances(got, cpu, start)}


CHECKS = [check_step_on_device, check_train_through_the_store, check_device_equals_cpu_to_rounding]


if __name__ == "__main__":
    fresh_process.main(CHECKS, extra={"measured": MEASURED})
