"""What the sample store's device checks (tests/*_gpu_checks.py) share: stores made of arrays and of game lines, minibatches
brought to the host and compared byte for byte, the host pipeline's first three arrays for given draws, hand-built SampleArrays,
move text and the golden game lines.  Imported by checks modules only, which run in a process of their own
(tests/fresh_process.py)."""
import json

import numpy as np

from ataxxzero_amd import link, training
from tests import aux_reference, helpers

F32 = np.float32
NAMES = ("features", "policy", "value", "ownership", "score", "reply", "aux_weight")


def host(out):
    return tuple(t.cpu().numpy() for t in out)


def same(got, want, what="", names=None, dtype=F32):
    """As many arrays, and each of one dtype (`dtype`, unless it is None), one shape and the same bytes.  `what`: the case, for
    the message (the callers pass it third); `names`: what to call the arrays, by default a minibatch's."""
    names = names or NAMES
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        name = names[k] if k < len(names) else k
        assert g.dtype == w.dtype and (dtype is None or g.dtype == dtype) and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)


def store_of(arrays, spare=0):
    """A store holding the SampleArrays, with room for `spare` more: one number, or (games, plies, targets)."""
    games, plies, targets = (spare,) * 3 if isinstance(spare, int) else spare
    store = link.SampleStore(len(arrays.games) + games, len(arrays.ply_flags) + plies, len(arrays.target_index) + targets)
    store.add_arrays(arrays)
    return store


def store_of_entries(entries, spare=0):
    return store_of(link.entries_to_arrays(entries), spare)


def arrays_of(games):
    """games: [(walls, [(mover stones, opponent stones, flags, target indices, target weights)] per ply)] -> link.SampleArrays;
    the mover of ply p is x on even plies.  Where every game's walls are None the arrays are made without wall masks."""
    rows, boards, flags, start, index, weight, masks = [], [], [], [0], [], [], []
    for walls, plies in games:
        rows.append((len(flags), len(plies), 1, 0))
        masks.append(walls)
        for p, (mover, opponent, f, t_index, t_weight) in enumerate(plies):
            boards.append((mover, opponent) if p % 2 == 0 else (opponent, mover))
            flags.append(f)
            index.extend(int(i) for i in t_index)
            weight.extend(float(w) for w in t_weight)
            start.append(len(index))
    return link.SampleArrays(rows, np.array(boards, dtype=np.uint64), flags, np.zeros(len(flags)), start,
                             np.array(index, dtype=np.uint16), np.array(weight, dtype=F32),
                             None if all(m is None for m in masks) else np.array(masks, dtype=np.uint64))


def all_pairs(store):
    """every (game, ply) the store holds"""
    games, _ = store.mirror()
    return np.array([(g, p) for g in range(len(games)) for p in range(int(games[g][1]))], dtype=np.int32)


def eligible_pairs(store):
    """the (game, ply) a draw may yield: the games' candidate plies that are neither a pass nor bad"""
    games, flags = store.mirror()
    cand, count, _, _ = store.ply_cum()
    return [(g, int(cand[int(games[g][0]) + k])) for g in range(len(games)) for k in range(int(count[g]))
            if not flags[int(games[g][0]) + int(cand[int(games[g][0]) + k])] & (link.SAMPLES_PLY_PASS | link.SAMPLES_PLY_BAD)]


def first_three(entries, draws, blend=0.0):
    """make_minibatch_reference's features, policy and value for given draws (game, ply, symmetry), sample by sample with the
    host pipeline's own functions."""
    feats, pols, vals = [], [], []
    for g, ply, s in draws:
        e = entries[g]
        mover = 1 + ply % 2
        feats.append(training.apply_symmetry(s, training.board_to_features(e["boards"][ply], mover, e.get("blockers"))))
        pols.append(training._policy_target(e, ply, s))
        vals.append([training._value_target(e, ply, mover, blend)])
    return np.asarray(feats, dtype=F32), np.asarray(pols, dtype=F32), np.asarray(vals, dtype=F32)


def restated(entries, draws, blend=0.0):
    """The seven arrays for draws (game, ply, symmetry): first_three's, and the four auxiliary ones of tests/aux_reference.py."""
    return first_three(entries, draws, blend) + aux_reference.batch(entries, draws)


def square_text(sq):
    return "abcdefg"[sq % 7] + "1234567"[sq // 7]


def move_text(mv):
    """the ring record's move word (from | to << 8, a clone from == to) as UAI text"""
    frm, to = mv & 0xFF, mv >> 8
    return square_text(to) if frm == to else square_text(frm) + square_text(to)


def golden_entries():
    with open(helpers.GOLDEN + "/train_entries.json") as f:
        return json.load(f)
