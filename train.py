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
--surprise-weight L draws a training game's plies by policy surprise, KL(policy target || prior of the --old-path network):
a share L of each game's sampling mass in proportion to it, the rest uniformly (implies --device-draws).
Entries written with the generator's --record-blockers carry "blockers", the wall cells of their board: every path then shows
them to the net in feature plane 3, and the surprise is measured over the moves the walls leave (no flag; without the key
nothing changes).
--aux-ownership, --aux-score and --aux-reply add auxiliary training targets (an extension): heads that exist only while training
predict who owns each cell at the game's end, the final margin in stones and the opponent's answer, from what the game lines
already hold; their weights go to NEW-PATH.aux.npz and the .npy file is what it always was.  All three 0 (the default):
nothing changes.
--reanalyse-fraction F searches that share of the training games' candidate plies again with the --old-path network before the
first step (--reanalyse-visits V each, --reanalyse-slots positions per round) and trains on the new visit distributions and
search values (MuZero's Reanalyse; an extension; implies --device-samples, needs --old-path).  F = 0 (the default): nothing
changes.
--prove-depth D runs the device's depth-D material alpha-beta search on the training games' stored plies before the first step
(--prove-nodes N nodes at most per ply; 0, the default, means no limit and is accepted up to depth 3): a ply the search proves
won or lost trains the value head on that outcome instead of the game's result, and with --prove-policy a ply proven won takes the
winning move as its policy target (what tablebase rescoring does for lc0; an extension; implies --device-samples, needs no
network).  D = 0 (the default): nothing changes.
--value-lambda L trains the value head of entries that carry "values" on TD(lambda) returns: an exponentially discounted average
of the search values of the plies that follow, closed with the game's result (KataGo's short-term value targets; an extension).
It works on every sample path; with a device store the pass runs after reanalysis and the proof pass, so refreshed values and
proven plies correct the targets of the plies before them.  Not together with --value-blend.  Absent (the default): nothing
changes.
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
    flag("--value-lambda", "L in [0, 1]: entries that carry \"values\" train the value head on their plies' TD(lambda) returns, "
                           "G_p = (1 - L) * values[p] + L * -G_{p+1}, closed with the game result at the last ply; with a device "
                           "store, plies proven by --prove-depth enter as +-1 (extension; not together with --value-blend; "
                           "absent: off)", type=float, default=None, metavar="L"),
    switch("--reference-bn-affine", "train batch-norm gamma/beta as the reference does and drop them on save "
                                    "(extension; see training.py)"),
    switch("--device-samples", "keep the games in device memory and build every minibatch with a HIP kernel: the same "
                               "minibatches, no per-step host work on the batch (extension; needs a GPU)"),
    switch("--device-draws", "with --device-samples (implied): the kernel also draws the samples, with Philox keyed by "
                             "123456789, instead of Python's random (extension)"),
    flag("--surprise-weight", "share L in [0, 1] of a game's sampling mass spread over its plies in proportion to the policy "
                              "surprise KL(target || prior of the --old-path network), the rest uniformly (extension; implies "
                              "--device-draws, needs --old-path; 0: off; KataGo uses 0.5)", type=float, default=0.0,
         metavar="L"),
    flag("--surprise-dtype", "tower precision of the surprise pass", default="bf16", choices=["f32", "bf16", "f16"],
         metavar="DTYPE"),
    flag("--aux-ownership", "weight A of the ownership loss: a head that exists only while training predicts, per cell, who owns "
                            "it at the game's end (games the rules adjudicate; extension, on every sample path; 0: off).  "
                            "KataGo weighs ownership 1.5 and the opponent's policy 0.15: a starting point, no value has been "
                            "tuned for Ataxx", type=float, default=0.0, metavar="A"),
    flag("--aux-score", "weight A of the score loss: the same head's prediction of the final margin in units of 49 stones "
                        "(extension; 0: off; not tuned for Ataxx)", type=float, default=0.0, metavar="A"),
    flag("--aux-reply", "weight A of the reply loss: a second training-only head predicts the policy target of the next ply, "
                        "the opponent's answer (extension; 0: off; KataGo: 0.15; not tuned for Ataxx)", type=float, default=0.0,
         metavar="A"),
    flag("--reanalyse-fraction", "share F in [0, 1] of the training games' candidate plies that are searched again with the "
                                 "--old-path network before the first step; their policy targets and values become the new "
                                 "roots' (extension; implies --device-samples, needs --old-path and --reanalyse-visits; 0: off)",
         type=float, default=0.0, metavar="F"),
    flag("--reanalyse-visits", "visits of each reanalysis search", type=int, default=0, metavar="V"),
    flag("--reanalyse-slots", "positions searched per round", type=int, default=4096, metavar="G"),
    flag("--reanalyse-dtype", "tower precision of the reanalysis searches", default="bf16", choices=["f32", "bf16", "f16"],
         metavar="DTYPE"),
    flag("--prove-depth", "depth D in 1 .. 8 of an alpha-beta search of the training games' stored plies before the first step; "
                          "a ply it proves won or lost trains the value head on the proven outcome (extension; implies "
                          "--device-samples; 0: off)", type=int, default=0, metavar="D"),
    flag("--prove-nodes", "node budget of that search per ply; 0: no limit, depth 1 .. 3 only, otherwise at least 256",
         type=int, default=0, metavar="N"),
    switch("--prove-policy", "with --prove-depth: a ply proven won takes the winning move as its policy target"),
]

if __name__ == "__main__":
    args = parse(__doc__.splitlines()[0], OPTIONS)
    surprise = {}
    if args.surprise_weight != 0.0:
        if not 0.0 < args.surprise_weight <= 1.0 or args.old_path is None:
            raise SystemExit("train.py: --surprise-weight takes L in [0, 1] and needs --old-path, the network the surprise "
                             "is measured against")
        surprise = {"surprise_weight": args.surprise_weight, "surprise_dtype": args.surprise_dtype}
        args.device_draws = True
    else:                                   # off: the run, and the line below, are those of a train.py without the flags
        del args.surprise_weight, args.surprise_dtype
    reanalysis = {}
    if args.reanalyse_fraction != 0.0:
        if not 0.0 < args.reanalyse_fraction <= 1.0 or args.reanalyse_visits < 1 or args.reanalyse_slots < 1 or \
                args.old_path is None:
            raise SystemExit("train.py: --reanalyse-fraction takes F in [0, 1], --reanalyse-visits V >= 1 (and --reanalyse-slots "
                             "G >= 1) and needs --old-path, the network the stored plies are searched with")
        reanalysis = {"reanalyse_fraction": args.reanalyse_fraction, "reanalyse_visits": args.reanalyse_visits,
                      "reanalyse_slots": args.reanalyse_slots, "reanalyse_dtype": args.reanalyse_dtype}
        args.device_samples = True
    else:                                   # off: as above
        del args.reanalyse_fraction, args.reanalyse_visits, args.reanalyse_slots, args.reanalyse_dtype
    proofs = {}
    if args.prove_depth != 0:
        why = training.prove_refusal(args.prove_depth, args.prove_nodes)
        if why:
            raise SystemExit("train.py: " + why)
        proofs = {"prove_depth": args.prove_depth, "prove_nodes": args.prove_nodes, "prove_policy": args.prove_policy}
        args.device_samples = True
    elif args.prove_nodes != 0 or args.prove_policy:
        raise SystemExit("train.py: --prove-nodes and --prove-policy need --prove-depth")
    else:                                   # off: as above
        del args.prove_depth, args.prove_nodes, args.prove_policy
    returns = {}
    if args.value_lambda is not None:
        why = training.value_lambda_refusal(args.value_lambda, args.value_blend)
        if why:
            raise SystemExit("train.py: " + why)
        returns = {"value_lambda": args.value_lambda}
    else:                                   # off: as above
        del args.value_lambda
    aux = {"aux_ownership": args.aux_ownership, "aux_score": args.aux_score, "aux_reply": args.aux_reply}
    if min(aux.values()) < 0.0:
        raise SystemExit("train.py: --aux-ownership, --aux-score and --aux-reply take weights >= 0")
    if not any(aux.values()):               # off: as above
        del args.aux_ownership, args.aux_score, args.aux_reply
        aux = {}
    print("Arguments:", args)
    training.train(args.games, args.old_path, args.new_path, steps=args.steps, minibatch_size=args.minibatch_size,
                   learning_rate=args.learning_rate, reference_bn_affine=args.reference_bn_affine, value_blend=args.value_blend,
                   device_samples=args.device_samples or args.device_draws, device_draws=args.device_draws, **surprise, **aux,
                   **reanalysis, **proofs, **returns)
