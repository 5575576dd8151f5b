#!/usr/bin/python
"""Trains a successor network from self-play game files on PyTorch-ROCm and writes it in the .npy layout.

Stands in for the reference's train.py: looper.py:140-148 runs
`python train.py --steps S --games G... --old-path A.npy --new-path B.npy`; the sample pipeline and optimiser
settings follow train.py:43-157 and live in ataxxzero_amd/training.py.  Entries written with the generator's playout cap on
carry "full" (one 0 / 1 per ply): samples are then drawn from the fully searched plies only (an extension; entries
without the key are sampled exactly as the reference does).  Entries written with --record-values or a resign threshold
carry "values", the search's own value at every ply: --value-blend L trains the value head on (1 - L) z + L values[ply]
instead of the game result z alone.  --device-samples keeps the games in device memory and lets a HIP kernel write every
minibatch into the trainer's tensors (the same minibatches; needs a GPU); --device-draws also draws the samples there.
"""
from ataxxzero_amd import training
from ataxxzero_amd.cli import flag, parse, switch

OPTIONS = [
    flag("--games", "self-play .json files to sample positions from", metavar="JSON", nargs="+", required=True),
    flag("--old-path", "network to start from (.npy); random initialisation when absent", metavar="NPY"),
    flag("--new-path", "where the trained network is written (.npy)", metavar="NPY", required=True),
    flag("--steps", "optimiser steps", type=int, default=1000, metavar="N"),
    flag("--minibatch-size", "positions per step", type=int, default=512, metavar="N"),
    flag("--learning-rate", "momentum-SGD learning rate", type=float, default=0.001, metavar="LR"),
    flag("--value-blend", "weight L of the search's recorded value in the value target, (1 - L) * z + L * values[ply], for "
                          "entries that carry \"values\" (extension; 0: the game result alone, as the reference)", type=float,
         default=0.0, metavar="L"),
    switch("--reference-bn-affine", "train batch-norm gamma/beta as the reference does and drop them on save "
                                    "(extension; see training.py)"),
    switch("--device-samples", "keep the games in device memory and build every minibatch with a HIP kernel: the same "
                               "minibatches, no per-step host work on the batch (extension; needs a GPU)"),
    switch("--device-draws", "with --device-samples (implied): the kernel also draws the samples, with Philox keyed by "
                             "123456789, instead of Python's random (extension)"),
]

if __name__ == "__main__":
    args = parse(__doc__.splitlines()[0], OPTIONS)
    print("Arguments:", args)
    training.train(args.games, args.old_path, args.new_path, steps=args.steps, minibatch_size=args.minibatch_size,
                   learning_rate=args.learning_rate, reference_bn_affine=args.reference_bn_affine, value_blend=args.value_blend,
                   device_samples=args.device_samples or args.device_draws, device_draws=args.device_draws)
