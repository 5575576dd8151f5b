#!/usr/bin/python
"""UAI engine over the GPU search: `python uai_interface.py --network-path X.npy [--visits N]`.

Stands in for the reference's script of the same name (command set uai_interface.py:41-88, options :97-100), so
any UAI master — the reference's unmodified uai_ringmaster.py included — can drive the net.  The dialogue itself
lives in ataxxzero_amd/uai.py (Session); the four codec helpers other reference modules import from here
(train.py:64-69, uai_ringmaster.py:42,59) are re-exported under their reference names.
"""
import argparse
import sys

from ataxxzero_amd.uai import square_to_xy as uai_decode_square
from ataxxzero_amd.uai import text_to_xy_move as uai_decode_move
from ataxxzero_amd.uai import xy_move_to_text as uai_encode_move
from ataxxzero_amd.uai import xy_to_square as uai_encode_square

__all__ = ["uai_encode_square", "uai_encode_move", "uai_decode_square", "uai_decode_move", "main"]


def main(options):
    from ataxxzero_amd import selfplay, uai
    selfplay.select_device(0)
    searcher = uai.Searcher(options.network_path, dtype=options.dtype, symmetry_average=options.symmetry_average,
                            parallel_leaves=options.parallel_leaves, virtual_loss=options.virtual_loss,
                            reuse_tree=options.reuse_tree, show_pv=options.show_pv, solver=options.solver,
                            random_symmetry=options.random_symmetry, fpu_reduction=options.fpu_reduction,
                            cpuct_base=options.cpuct_base, cpuct_init=options.cpuct_init)
    session = uai.Session(searcher, visits=options.visits, safety_ms=options.safety_ms, show_game=options.show_game,
                          log=sys.stderr)
    session.serve(sys.stdin, sys.stdout)


if __name__ == "__main__":
    cli = argparse.ArgumentParser(description="UAI engine: MCTS and the policy/value net on one MI355X.")
    cli.add_argument("--network-path", required=True, metavar="NPY", help=".npy weight file in the model.py layout")
    cli.add_argument("--visits", type=int, default=None, metavar="N", help="search exactly N steps per move instead of using the clock")
    cli.add_argument("--safety-ms", type=int, default=0, metavar="MS", help="margin subtracted from every movetime")
    cli.add_argument("--show-game", action="store_true", help="echo positions set by `position fen` to stderr")
    cli.add_argument("--symmetry-average", action="store_true", help="evaluate every position as the mean over its 8 dihedral images (nn_evals.py:48-62; extension)")
    cli.add_argument("--random-symmetry", action="store_true",
                     help="evaluate every position under one of the 8 symmetries of the board, drawn per position (extension; "
                          "AlphaZero's leaf evaluation): no extra tower work.  Not with --symmetry-average")
    cli.add_argument("--parallel-leaves", type=int, default=1, metavar="K",
                     help="leaves per search iteration, 1..64, spread by a virtual loss and evaluated in one tower launch "
                          "(extension; 1 = the reference's one-leaf search)")
    cli.add_argument("--virtual-loss", type=int, default=1, metavar="V",
                     help="visits of virtual loss per path on every edge it takes, 1..16 (with --parallel-leaves > 1)")
    cli.add_argument("--reuse-tree", action="store_true",
                     help="keep the search tree across moves: the subtree of the moves played is inherited when the new position "
                          "is the old root or one or two moves below it (engine.py:452-472); --visits N then means N MORE steps")
    cli.add_argument("--show-pv", action="store_true",
                     help="before bestmove, print `info nodes <root visits> inherited <n> score <q> pv <moves>`")
    cli.add_argument("--solver", action="store_true",
                     help="prove wins and losses in the search tree (MCTS-solver; extension): a proven winning move is played "
                          "without sampling (`info string proven win`), a timed search stops once the root is proven")
    cli.add_argument("--fpu-reduction", type=float, default=None, metavar="R",
                     help="first-play urgency (extension, off by default): an unvisited move scores its parent's mean score "
                          "less R * sqrt(policy mass of the visited moves), not 0, R >= 0 (Leela's reduction; 0.25 is a "
                          "starting point, nothing is tuned for Ataxx)")
    cli.add_argument("--cpuct-base", type=float, default=None, metavar="B",
                     help="an exploration rate that grows with the visits (extension, off by default): c = log((1 + N + B) / B) "
                          "+ C in the place of the constant 1.0, B > 0.  AlphaZero's published 19652 with --cpuct-init 1.25 is "
                          "a starting point; nothing is tuned for Ataxx")
    cli.add_argument("--cpuct-init", type=float, default=0.0, metavar="C", help="the C of --cpuct-base (ignored without it)")
    cli.add_argument("--dtype", default="f16", choices=["bf16", "f16", "f32"],
                     help="tower arithmetic (extension).  Match play defaults to f16: with a trained net the f16 search picks "
                          "the f32 search's move in 100 %% of test positions, bf16 in 96 %% (DESIGN.md section 5); bf16 is 3-6 %% faster")
    options = cli.parse_args()
    if options.random_symmetry and options.symmetry_average:
        cli.error("--random-symmetry and --symmetry-average exclude each other")
    if (options.fpu_reduction is not None or options.cpuct_base is not None) and options.symmetry_average:
        cli.error("--fpu-reduction and --cpuct-base are not available with --symmetry-average")
    print(options, file=sys.stderr)
    main(options)
