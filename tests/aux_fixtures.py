"""Games for the tests of the auxiliary targets (tests/test_aux_host.py, tests/aux_gpu_checks.py): the golden training
entries, games played to their end on boards with walls by tests/walls_fixtures.py's random player, cuts of them, and ring
records written by hand from the same games."""
import copy
import json

import numpy as np

from ataxxzero_amd import link
from tests import helpers
from tests import rules_reference as rr
from tests import walls_fixtures as wf

PLIES_CUT = 20


def golden_entries():
    with open(helpers.GOLDEN + "/train_entries.json") as f:
        return json.load(f)


_PLAYED = {}


def played(fen, seed):
    """One game played to its end (at most 400 plies) -> (entry, positions), once per process."""
    if (fen, seed) not in _PLAYED:
        _PLAYED[(fen, seed)] = wf.play_game(fen, seed, max_plies=400)
    return _PLAYED[(fen, seed)]


def walled_games():
    """[(entry, positions)]: three games on the default wall map and three on the asymmetric one."""
    return [played(wf.DEFAULT_FEN, s) for s in (100, 101, 102)] + [played(wf.ASYMMETRIC_FEN, s) for s in (100, 101, 102)]


def cut(entry, plies=PLIES_CUT):
    """The first `plies` plies of a game line: a truncated file."""
    out = {k: (v[:plies] if k in ("boards", "moves", "dists", "full", "values") else copy.deepcopy(v)) for k, v in entry.items()}
    return out


def with_full(entry, every=3):
    """The line with "full": every `every`-th ply was searched in full."""
    out = dict(entry)
    out["full"] = [1 if p % every == 0 else 0 for p in range(len(entry["boards"]))]
    return out


def mixed_entries():
    """Entries of every flavour the auxiliary targets meet: golden games (with dists, with list-typed moves, with
    random_ply), walled games ended by the rules, cuts without owners, a game with "full", and a one-ply game."""
    walled = [e for e, _ in walled_games()]
    return (golden_entries() + walled + [cut(walled[0]), cut(walled[3]), with_full(walled[1]), with_full(cut(walled[4], 31), 2),
                                         cut(walled[2], 1)])


def record_of(entry, positions, uid=0):
    """The ring record of a game of walls_fixtures.play_game that has no pass: boards and moves from its positions, the
    targets' counts the 64ths its "dists" are made of."""
    plies = len(positions)
    assert "pass" not in entry["moves"]
    words = [link.RECORD_MAGIC, 0, uid, plies, entry["result"], 0, 0, 0]
    for p, board in enumerate(positions):
        x, o, _ = board.masks()
        assert board.turn == p % 2
        dist = entry["dists"][p]
        words += [x & 0xFFFFFFFF, x >> 32, o & 0xFFFFFFFF, o >> 32, rr.move_from_string(entry["moves"][p]) | len(dist) << 16, 0]
        words += [rr.move_from_string(m) | int(round(w * 64)) << 16 for m, w in dist.items()]
    words[link.REC_WORDS] = len(words)
    return np.array(words, dtype=np.uint32)


def passless_games(fen, count, first_seed=100):
    """The first `count` games from `fen` in which nobody had to pass -> [(entry, positions)]."""
    out, seed = [], first_seed
    while len(out) < count:
        entry, positions = played(fen, seed)
        if "pass" not in entry["moves"]:
            out.append((entry, positions))
        seed += 1
    return out
