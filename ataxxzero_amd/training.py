"""Training side of the loop on PyTorch-ROCm (reference train.py + model.py's training graph).

Sample pipeline restated from train.py:11-89 (random game, random ply, side to move from ply
parity, value target +-1, one of the 8 dihedral symmetries, policy target from `dists` or a
one-hot of the move played), drawing from Python's `random` in the reference's order so the
same games file gives the same minibatches.  Loss and optimiser from model.py:81-101: softmax
cross-entropy on the 833 move logits + value MSE + 1e-4 * l2_loss over the trainable variables,
Momentum(0.9).  The trained net is written in the reference's `.npy` layout (model.py:179-183).

Q1: the reference trains batch-norm gamma/beta but never saves them, so
the net it plays with is not the net it trained.  Here gamma = 1, beta = 0 are fixed
(`affine=False`) by default — what is saved is exactly what was trained; `reference_bn_affine=True`
restores the reference's train-then-drop behaviour.
"""
import json
import os
import random

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import model

BOARD = model.BOARD_SIZE
MOVE_TYPES = model.MOVE_TYPES
# engine.py:75: layer of a jump = rank of (dx, dy) among the distance-2 offsets (ataxx_rules.py:17-20)
FAR_OFFSETS = [(a, b) for a in (-2, -1, 0, 1, 2) for b in (-2, -1, 0, 1, 2)
               if (a, b) != (0, 0) and (a, b) not in [(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1)]]
DELTA_LAYER = {d: i for i, d in enumerate(FAR_OFFSETS)}


# ---------------------------------------------------------------- sample pipeline (train.py:11-89)

def uai_decode_move(text):
    """UAI text -> the reference's move value ("pass" | ("c", (x, y)) | ((x0, y0), (x1, y1)))."""
    from .uai import text_to_xy_move
    return text_to_xy_move(text)


def board_to_features(cells, to_move, blockers=None):
    """Four planes [x][y][c] — ones, mover's stones, opponent's stones, blockers — from the 49 recorded cells (index
    x + 7 y), engine.py:53-73.  blockers: the wall cells in that index (an entry's "blockers"; the reference's files carry
    none and its plane stays zero)."""
    grid = np.asarray(cells, dtype=np.int8).reshape(BOARD, BOARD).T      # grid[x, y]
    planes = np.zeros((BOARD, BOARD, 4), dtype=np.int8)
    planes[..., 0] = 1
    planes[..., 1] = grid == to_move
    planes[..., 2] = (grid != 0) & (grid != to_move)
    if blockers:
        planes[..., 3] = _wall_row(blockers).reshape(BOARD, BOARD).T
    return planes


def _wall_row(blockers):
    """The wall cells of an entry's "blockers" as 49 int8 in the index of its boards."""
    row = np.zeros(BOARD * BOARD, dtype=np.int8)
    row[np.asarray(blockers, dtype=np.int64)] = 1
    return row


def check_blockers(entry, name):
    """ValueError naming the game unless the entry's "blockers" (if it has any) is a strictly ascending list of cells in
    0..48 none of which ever holds a stone."""
    if "blockers" not in entry:
        return
    cells = entry["blockers"]
    if (not isinstance(cells, list) or any(type(c) is not int or not 0 <= c < BOARD * BOARD for c in cells) or
            any(a >= b for a, b in zip(cells, cells[1:]))):
        raise ValueError("%s: \"blockers\" must be an ascending list of distinct cells in 0..48, not %r" % (name, cells))
    if cells:
        boards = np.asarray(entry["boards"], dtype=np.int8).reshape(-1, BOARD * BOARD)
        on = np.flatnonzero((boards[:, cells] != 0).any(axis=1))
        if len(on):
            raise ValueError("%s: a stone stands on a wall cell at ply %d" % (name, int(on[0])))


def _symmetry_bits(index):
    if not 0 <= index < 8:
        raise ValueError("symmetry index %r" % (index,))
    return bool(index & 1), bool(index & 2), bool(index & 4)


def apply_symmetry(index, arr):
    """The dihedral symmetry `index` of train.py:11-23 on an [x][y][c] array: bit 0 mirrors x, bit 1 mirrors y,
    bit 2 then transposes; always a fresh array."""
    flip_x, flip_y, transpose = _symmetry_bits(index)
    out = np.array(arr)
    if flip_x:
        out = np.flip(out, axis=0)
    if flip_y:
        out = np.flip(out, axis=1)
    if transpose:
        out = np.transpose(out, (1, 0, 2))
    return np.ascontiguousarray(out)


def apply_symmetry_to_move(index, move):
    """The same symmetry on a move value (train.py:25-40)."""
    flip_x, flip_y, transpose = _symmetry_bits(index)
    last = BOARD - 1

    def image(xy):
        x = last - xy[0] if flip_x else xy[0]
        y = last - xy[1] if flip_y else xy[1]
        return (y, x) if transpose else (x, y)

    return tuple(part if part == "c" else image(part) for part in move)


def add_move_to_heatmap(heatmap, move, coef=1):
    """Policy plane of a move: clones in the last layer of the destination cell, jumps in the layer of their
    (dx, dy) (engine.py:75-87)."""
    source, (tx, ty) = move
    layer = MOVE_TYPES - 1 if source == "c" else DELTA_LAYER[(tx - source[0], ty - source[1])]
    heatmap[tx, ty, layer] += coef


def _policy_target(entry, ply, symmetry_index):
    target = np.zeros((BOARD, BOARD, MOVE_TYPES), dtype=np.float32)
    if "dists" in entry:
        weighted = entry["dists"][ply].items()
    else:
        weighted = [(entry["moves"][ply], 1)]       # one-hot on the move played (random / teacher games)
    for mv, weight in weighted:
        if isinstance(mv, str):
            mv = uai_decode_move(mv)
        else:                                       # json turned the tuples into lists
            mv = (mv[0] if mv[0] == "c" else tuple(mv[0]), tuple(mv[1]))
        add_move_to_heatmap(target, apply_symmetry_to_move(symmetry_index, mv), weight)
    if abs(1 - target.sum()) >= 1e-3:
        raise AssertionError("policy target does not sum to one")
    return target


def _draw_ply(entry):
    """The ply a sample of `entry` is taken from, or None if the entry has none to give.  An entry of a generator run with
    the playout cap carries "full" (one 0 / 1 per ply): only its FULL plies — searched with the whole budget and root
    noise — are policy targets, so the ply is drawn among those, and an entry without one is skipped.  Every other entry
    draws exactly as the reference does (train.py:46)."""
    if "full" not in entry:
        return random.randrange(len(entry["boards"]))
    full = [p for p, f in enumerate(entry["full"]) if f]
    return full[random.randrange(len(full))] if full else None


def lambda_returns(values, result, lam, proofs=None):
    """The TD(lambda) returns G_p of one game in Python floats (include/ataxxzero_hip.h, "lambda-returns as value targets"):
    values the search's value of every ply for its mover, result the game's (1: x, 2: o, 0: none), lam in [0, 1], proofs one
    word per ply (0: none) or None.  From the last ply down: next = z_p at the last ply and -G_{p+1} before it, then
    a = 1.0 - lam, b = a * v_p, c = lam * next, G_p = b + c — four operations in this order — and +-1.0 where the ply is proven."""
    out = [0.0] * len(values)
    a = 1.0 - lam
    nxt = 0.0
    for p in range(len(values) - 1, -1, -1):
        if p == len(values) - 1:
            nxt = 1.0 if result == 1 + p % 2 else -1.0
        b = a * float(values[p])
        c = lam * nxt
        g = b + c
        if proofs is not None and proofs[p] != 0:
            g = 1.0 if proofs[p] > 0 else -1.0
        out[p] = g
        nxt = -g
    return out


_RETURNS = {}             # id(entry) -> (entry, lambda, returns): bounded like _ARRAYS


def _entry_returns(entry, lam):
    """lambda_returns of an entry that carries "values", computed once per (entry, lambda)."""
    row = _RETURNS.get(id(entry))
    if row is None or row[0] is not entry or row[1] != lam:
        if len(_RETURNS) >= _ARRAYS_MAX:
            for key in list(_RETURNS)[:_ARRAYS_MAX // 10]:
                del _RETURNS[key]
        values = entry["values"][:len(entry["boards"])]                   # the plies the store keeps (link.entries_to_arrays)
        row = _RETURNS[id(entry)] = (entry, lam, lambda_returns(values, entry["result"], lam))
    return row[2]


def value_lambda_refusal(value_lambda, value_blend):
    """Why train.py --value-lambda L is refused, or None."""
    if value_blend != 0.0:
        return "--value-lambda and --value-blend are two value targets: give one of them"
    if not 0.0 <= value_lambda <= 1.0:
        return "--value-lambda must lie in [0, 1]"
    return None


def _value_target(entry, ply, mover, value_blend, value_lambda=None):
    """The value target of a sample: the game result z seen by the mover, +-1 — or, with value_blend = L != 0 and an entry that
    carries "values" (the search's own value at every ply, the mover's expectation in [-1, 1]), the blend
    (1 - L) * z + L * values[ply] in Python floats — or, with value_lambda = L (not None) and such an entry, the ply's
    lambda-return (lambda_returns); an entry without "values" keeps z."""
    z = 1 if entry["result"] == mover else -1
    if value_lambda is not None and "values" in entry:
        return _entry_returns(entry, value_lambda)[ply]
    if value_blend and "values" in entry:
        return (1 - value_blend) * z + value_blend * entry["values"][ply]
    return z


_OWNERS = {}              # id(entry) -> (entry, owner row): bounded like _ARRAYS


def _entry_owner_row(entry):
    """The owners of an entry's final position (link.entry_owners; include/ataxxzero_hip.h, "Auxiliary targets") as 49 int8 in
    the index of its boards: +1 where x owns the cell, -1 where o does, 0 on walls — or None when the game has no owners."""
    row = _OWNERS.get(id(entry))
    if row is None or row[0] is not entry:
        from . import link
        own_x, own_o = link.entry_owners(entry)
        cells = None
        if own_x | own_o:
            bits = [c % BOARD + BOARD * (BOARD - 1 - c // BOARD) for c in range(BOARD * BOARD)]
            cells = np.array([((own_x >> b) & 1) - ((own_o >> b) & 1) for b in bits], dtype=np.int8)
        if len(_OWNERS) >= _ARRAYS_MAX:
            for key in list(_OWNERS)[:_ARRAYS_MAX // 10]:
                del _OWNERS[key]
        row = _OWNERS[id(entry)] = (entry, cells)
    return row[1]


def _reply_present(entry, ply):
    """Is ply + 1 one a sample could have been drawn from (its target is then checked like any sample's)?"""
    nxt = ply + 1
    return (nxt < len(entry["boards"]) and entry["moves"][nxt] != "pass" and
            ("full" not in entry or bool(entry["full"][nxt])))


def aux_targets(entry, ply, symmetry):
    """The auxiliary targets of the sample (entry, ply, symmetry) -> (ownership (7, 7), score (1,), reply (7, 7, 17),
    aux_weight (2,)), float32, from the entry alone (include/ataxxzero_hip.h, "Auxiliary targets"): the final owners seen by
    the mover under the symmetry, their margin, the policy target of ply + 1, and which of the two the sample has."""
    mover = 1 + ply % 2
    owners = _entry_owner_row(entry)
    ownership = np.zeros((BOARD, BOARD), dtype=np.float32)
    score = np.zeros(1, dtype=np.float32)
    weight = np.zeros(2, dtype=np.float32)
    if owners is not None:
        seen = owners if mover == 1 else -owners
        ownership = apply_symmetry(symmetry, seen.reshape(BOARD, BOARD).T[..., None])[..., 0].astype(np.float32)
        score[0] = int(seen.sum())
        weight[0] = 1.0
    reply = np.zeros((BOARD, BOARD, MOVE_TYPES), dtype=np.float32)
    if _reply_present(entry, ply):
        try:
            reply = _policy_target(entry, ply + 1, symmetry)
            weight[1] = 1.0
        except AssertionError:                      # a bad ply: no sample is drawn from it, and it is nobody's reply
            pass
    return ownership, score, reply, weight


def _draw_sample(entries):
    """(entry, ply, symmetry) of one sample.  The draws from `random` come in the reference's order — game, ply,
    symmetry (train.py:45-60)."""
    while True:
        entry = random.choice(entries)
        ply = _draw_ply(entry)
        if ply is None:
            continue
        if "random_ply" in entry:                   # ONE_RANDOM_MOVE games: the position right after the random move
            ply = entry["random_ply"] + 1
        if entry["moves"][ply] == "pass":
            continue
        return entry, ply, random.randrange(8)


def get_sample_from_entries(entries, value_blend=0.0, aux=False, value_lambda=None):
    """One training sample (train.py:43-77).  The draws from `random` come in the reference's order — game, ply,
    symmetry — so a games file yields the same minibatches as there.  aux: the sample's aux_targets behind the three.
    value_lambda: _value_target."""
    entry, ply, symmetry_index = _draw_sample(entries)
    mover = 1 + ply % 2                             # x (1) moves on even plies
    features = apply_symmetry(symmetry_index, board_to_features(entry["boards"][ply], mover, entry.get("blockers")))
    value = [_value_target(entry, ply, mover, value_blend, value_lambda)]
    sample = features, _policy_target(entry, ply, symmetry_index), value
    return sample + aux_targets(entry, ply, symmetry_index) if aux else sample


def load_entries(paths):
    entries = []                                                          # train.py:79-89
    for path in paths:
        with open(path) as f:
            for number, line in enumerate(f, 1):
                line = line.strip()
                if line:
                    entries.append(json.loads(line))
                    check_blockers(entries[-1], "%s, line %d" % (path, number))
    random.shuffle(entries)
    return entries


def make_minibatch_reference(entries, size, value_blend=0.0, aux=False, value_lambda=None):
    """`size` samples drawn one by one with get_sample_from_entries (train.py:123-130).  aux: seven arrays, the samples'
    aux_targets (ownership, score, reply, aux_weight) behind the three; `random` is consumed as without it."""
    columns = [[] for _ in range(7 if aux else 3)]
    for _ in range(size):
        for column, part in zip(columns, get_sample_from_entries(entries, value_blend, aux, value_lambda)):
            column.append(part)
    return tuple(np.asarray(column, dtype=np.float32) for column in columns)


def _symmetry_tables():
    """For each of the 8 symmetries: which recorded cell (index x + 7 y) every feature cell [x][y] shows, and where every
    flat policy index 119 x + 17 y + layer goes — both read off apply_symmetry / apply_symmetry_to_move themselves."""
    cell_of = np.arange(BOARD * BOARD, dtype=np.int64).reshape(BOARD, BOARD).T[..., None]      # [x][y] -> x + 7 y
    cell_src = np.stack([apply_symmetry(s, cell_of)[..., 0].reshape(-1) for s in range(8)])       # [s][x * 7 + y]
    policy_to = np.zeros((8, BOARD * BOARD * MOVE_TYPES), dtype=np.int64)
    probe = np.zeros((BOARD, BOARD, MOVE_TYPES))

    def flat(move):
        probe[...] = 0
        add_move_to_heatmap(probe, move)
        return int(np.flatnonzero(probe.ravel())[0])

    for x in range(BOARD):
        for y in range(BOARD):
            moves = [("c", (x, y))] + [((x - dx, y - dy), (x, y)) for dx, dy in FAR_OFFSETS
                                       if 0 <= x - dx < BOARD and 0 <= y - dy < BOARD]
            for m in moves:
                for s in range(8):
                    policy_to[s, flat(m)] = flat(apply_symmetry_to_move(s, m))
    return cell_src, policy_to


_TABLES = None
# Per-entry arrays of the batched pipeline, kept OUTSIDE the entries (they stay plain JSON data) and bounded: keyed by
# id(entry) with the entry itself held, so an id is never reused while its row is alive; oldest rows go first.
_ARRAYS = {}
_ARRAYS_MAX = 100000      # entries; about 15 KB each (int8 cells, int16 indices, float32 weights)


_FLAT_INDEX = {}          # move as the entry spells it (UAI text, or json's nested lists as tuples) -> flat policy index


def _flat_policy_index(mv):
    """Flat index 119 x + 17 y + layer of a move's cell in the policy heat map, through add_move_to_heatmap itself, once per
    distinct move (there are 529): a games file names the same few hundred moves millions of times."""
    key = mv if isinstance(mv, str) else (mv[0] if mv[0] == "c" else tuple(mv[0]), tuple(mv[1]))
    flat = _FLAT_INDEX.get(key)
    if flat is None:
        probe = np.zeros((BOARD, BOARD, MOVE_TYPES))
        add_move_to_heatmap(probe, uai_decode_move(key) if isinstance(key, str) else key)
        flat = _FLAT_INDEX[key] = int(np.flatnonzero(probe.ravel())[0])
    return flat


def _entry_arrays(entry):
    """Per-entry arrays for the batched pipeline, built on first use: cells [plies][49] and, per ply, the flat policy
    indices and weights of its target (the visit distribution, or the move played)."""
    row = _ARRAYS.get(id(entry))
    cache = row[1] if row is not None and row[0] is entry else None
    if cache is None:
        cells = np.asarray(entry["boards"], dtype=np.int8)
        idx, wts, start = [], [], [0]
        for ply in range(len(entry["boards"])):
            if "dists" in entry:
                items = entry["dists"][ply].items()
            else:
                items = [(entry["moves"][ply], 1)]
            for mv, w in items:
                if mv == "pass":
                    continue
                idx.append(_flat_policy_index(mv))
                wts.append(w)
            start.append(len(idx))
        cache = (cells, np.asarray(idx, dtype=np.int16), np.asarray(wts, dtype=np.float32),
                 np.asarray(start, dtype=np.int32))
        if len(_ARRAYS) >= _ARRAYS_MAX:
            for key in list(_ARRAYS)[:_ARRAYS_MAX // 10]:
                del _ARRAYS[key]
        _ARRAYS[id(entry)] = (entry, cache)
    return cache


def make_minibatch(entries, size, value_blend=0.0, aux=False, value_lambda=None):
    """The same `size` samples as make_minibatch_reference — same draws from `random` in the same order, bit-identical
    arrays (tests/test_training.py) — assembled with array operations instead of per-sample Python: the sample pipeline,
    not the GPU step, bounded train.py's rate.  value_blend, value_lambda: _value_target.  aux: seven arrays, as
    make_minibatch_reference."""
    global _TABLES
    if _TABLES is None:
        _TABLES = _symmetry_tables()
    cell_src, policy_to = _TABLES
    cells, movers, syms, targets, rows, pidx, pw, walls = [], [], [], [], [], [], [], {}
    owned, r_rows, r_idx, r_w = {}, [], [], []
    while len(cells) < size:
        entry = random.choice(entries)                      # the reference's draws, in its order (train.py:45-60)
        ply = _draw_ply(entry)
        if ply is None:
            continue
        if "random_ply" in entry:
            ply = entry["random_ply"] + 1
        if entry["moves"][ply] == "pass":
            continue
        sym = random.randrange(8)
        c, idx, wts, start = _entry_arrays(entry)
        lo, hi = start[ply], start[ply + 1]
        rows.append(np.full(hi - lo, len(cells), dtype=np.int64))
        pidx.append(policy_to[sym, idx[lo:hi]])
        pw.append(wts[lo:hi])
        if entry.get("blockers"):
            walls[len(cells)] = _wall_row(entry["blockers"])
        if aux:
            owners = _entry_owner_row(entry)
            if owners is not None:
                owned[len(cells)] = owners if ply % 2 == 0 else -owners
            if _reply_present(entry, ply):
                lo, hi = start[ply + 1], start[ply + 2]
                r_rows.append(np.full(hi - lo, len(cells), dtype=np.int64))
                r_idx.append(policy_to[sym, idx[lo:hi]])
                r_w.append(wts[lo:hi])
        cells.append(c[ply])
        movers.append(1 + ply % 2)
        syms.append(sym)
        targets.append(_value_target(entry, ply, 1 + ply % 2, value_blend, value_lambda))
    cells = np.stack(cells)
    movers = np.asarray(movers, dtype=np.int8)[:, None]
    shown = np.take_along_axis(cells, cell_src[np.asarray(syms)], axis=1)        # [b][x * 7 + y]
    feats = np.zeros((size, BOARD * BOARD, 4), dtype=np.float32)
    feats[..., 0] = 1
    feats[..., 1] = shown == movers
    feats[..., 2] = (shown != 0) & (shown != movers)
    for i, row in walls.items():                            # plane 3: the walls, under the sample's symmetry like the stones
        feats[i, :, 3] = row[cell_src[syms[i]]]
    pols = np.zeros((size, BOARD * BOARD * MOVE_TYPES), dtype=np.float32)
    np.add.at(pols, (np.concatenate(rows), np.concatenate(pidx)), np.concatenate(pw))
    if (np.abs(1 - pols.sum(axis=1)) >= 1e-3).any():
        raise AssertionError("policy target does not sum to one")
    vals = np.asarray(targets, dtype=np.float32)[:, None]
    batch = feats.reshape(size, BOARD, BOARD, 4), pols.reshape(size, BOARD, BOARD, MOVE_TYPES), vals
    if not aux:
        return batch
    ownership = np.zeros((size, BOARD * BOARD), dtype=np.float32)
    score = np.zeros((size, 1), dtype=np.float32)
    weight = np.zeros((size, 2), dtype=np.float32)
    for i, seen in owned.items():                           # the owners as the mover sees them, under the sample's symmetry
        ownership[i] = seen[cell_src[syms[i]]]
        score[i, 0] = int(seen.sum())
        weight[i, 0] = 1.0
    replies = np.zeros((size, BOARD * BOARD * MOVE_TYPES), dtype=np.float32)
    if r_rows:
        np.add.at(replies, (np.concatenate(r_rows), np.concatenate(r_idx)), np.concatenate(r_w))
        weight[np.unique(np.concatenate(r_rows)), 1] = 1.0
    for i in np.flatnonzero(np.abs(1 - replies.sum(axis=1)) >= 1e-3):     # a bad ply (or no ply) is nobody's reply
        replies[i] = 0
        weight[i, 1] = 0.0
    return batch + (ownership.reshape(size, BOARD, BOARD), score, replies.reshape(size, BOARD, BOARD, MOVE_TYPES), weight)


# ---------------------------------------------------------------- device-resident samples (link.SampleStore)

AUX_SEED = 987654321                  # numpy's PCG64 seed of freshly initialised auxiliary heads (Network(aux_heads=True))
DEVICE_DRAW_SEED = 123456789          # train.py --device-draws: the Philox key of the draws made on the device


def _draw_tables(store):
    """The store's host mirror as plain Python values, built once per state of the store: per game (first ply, plies, has
    "full", random_ply + 1), the ply flags as bytes, and the full plies of the games that carry "full" (on first use)."""
    from . import link
    mirror = store.mirror()
    tables = getattr(store, "_draw_tables", None)
    if tables is None or tables[0] is not mirror:
        games = [(int(a), int(n), bool(w & link.SAMPLES_GAME_HAS_FULL), int(r)) for a, n, w, r in mirror[0]]
        tables = store._draw_tables = (mirror, games, mirror[1].tobytes(), {})
    return tables[1:]


def make_minibatch_device(store, first_game, n_games, size, value_blend=0.0, out=None, draws="reference", seed=DEVICE_DRAW_SEED,
                          step=0, aux=False):
    """`size` samples of the games [first_game, first_game + n_games) of a link.SampleStore, written by its kernel into the three
    GPU tensors `out` (fresh ones by default) -> out.  draws="reference": Python's `random` is consumed exactly as make_minibatch
    consumes it for entries[first_game:first_game + n_games] — game, ply among the candidates, the random_ply replacement, the
    pass rejection, symmetry — so the same games give the same minibatches, bit for bit; draws="device": the kernel draws with
    Philox keyed by `seed` at counter `step` (SampleStore.draw_gather).  aux: seven tensors, the auxiliary targets behind the
    three (SampleStore.aux_outputs), for the same draws."""
    if draws == "device":
        return store.draw_gather(size, seed, step, first_game, n_games, value_blend, out=out, aux=aux)
    if draws != "reference":
        raise ValueError("draws must be \"reference\" or \"device\"")
    from . import link
    games, flags, full_plies = _draw_tables(store)
    choices = range(first_game, first_game + n_games)
    rows = []
    while len(rows) < size:
        g = random.choice(choices)                          # the reference's draws, in its order (train.py:45-60)
        first, plies, has_full, random_ply_1 = games[g]
        if not has_full:
            ply = random.randrange(plies)
        else:
            full = full_plies.get(g)
            if full is None:
                full = full_plies[g] = [p for p in range(plies) if flags[first + p] & link.SAMPLES_PLY_FULL]
            if not full:
                continue
            ply = full[random.randrange(len(full))]
        if random_ply_1:
            ply = random_ply_1
            if ply >= plies:
                raise IndexError("random_ply + 1 = %d in a game of %d plies" % (ply, plies))
        if flags[first + ply] & link.SAMPLES_PLY_PASS:
            continue
        rows.append((g, ply, random.randrange(8)))
    return store.gather(np.asarray(rows, dtype=np.int32), value_blend, out=out, aux=aux)


def _fill_store(entries, log, aux=False, reanalyse_fraction=0.0, n_test=10, prove_policy=False):
    """reanalyse_fraction F > 0: the store gets round(F * C) * MAX_MOVES targets of head-room, C the candidate plies of the
    training games [n_test, n) that are no passes (reanalysed targets are appended: SampleStore.retarget).  prove_policy: C
    more, one per ply a proof pass can retarget (SampleStore.prove)."""
    from . import link
    link.require_gpu()
    arrays = link.entries_to_arrays(entries, aux=aux)
    spare = 0
    if reanalyse_fraction > 0.0 or prove_policy:
        c = 0
        for first, plies, word, _ in arrays.games[n_test:].tolist():
            f = arrays.ply_flags[first:first + plies]
            cand = (f & link.SAMPLES_PLY_FULL) != 0 if word & link.SAMPLES_GAME_HAS_FULL else np.ones(plies, dtype=bool)
            c += int((cand & ((f & link.SAMPLES_PLY_PASS) == 0)).sum())
        spare = round(reanalyse_fraction * c) * link.MAX_MOVES + (c if prove_policy else 0)
        if len(arrays.target_index) + spare >= 1 << 31:
            raise ValueError("--reanalyse-fraction %g%s of %d plies asks for %d targets of head-room: a store holds fewer than "
                             "2^31" % (reanalyse_fraction, " and --prove-policy" if prove_policy else "", c, spare))
    store = link.SampleStore(max(len(arrays.games), 1), max(len(arrays.ply_flags), 1), max(len(arrays.target_index) + spare, 1))
    store.add_arrays(arrays)
    c = store.counts()
    masks = store.game_blockers()
    walled = masks[masks != 0]
    log("Device samples: %i games, %i plies, %i policy targets in device memory; %i plies whose target does not sum to one%s."
        % (c["games"], c["plies"], c["targets"], c["bad_plies"],
           "; %i games on %i wall maps" % (len(walled), len(set(walled.tolist()))) if len(walled) else ""))
    return store


def surprise_weights(kl, games, candidate_lists, lam):
    """Policy surprise weighting (Wu 2019, section 3.3) -> one float64 weight per ply.  kl: the surprise of every ply of the
    games; games: rows (first ply, plies, ...) with the first ply counted from kl[0]; candidate_lists: per game the plies a
    sample may be drawn from.  A game with n candidates spreads the mass n over them, (1 - lam) of it uniformly and lam in
    proportion to the surprise: w_i = (1 - lam) + lam * n * KL_i / sum KL; every w_i = 1 where the sum is 0; 0 elsewhere."""
    kl = np.asarray(kl, dtype=np.float64)
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError("the surprise weight must lie in [0, 1]")
    w = np.zeros(len(kl), dtype=np.float64)
    for row, cand in zip(games, candidate_lists):
        at = int(row[0]) + np.asarray(cand, dtype=np.int64)
        if not len(at):
            continue
        total = kl[at].sum()
        w[at] = (1.0 - lam) + lam * len(at) * kl[at] / total if total > 0.0 else 1.0
    return w


def _apply_surprise(store, old_path, lam, dtype, n_test, log):
    """One surprise pass over the training games [n_test, games) against the net at old_path, then the ply weights."""
    import time
    from . import link
    cw, bnp = model.load_model(old_path)
    net = link.Net(cw, bnp)
    games, _ = store.mirror()
    count = len(games) - n_test
    t0 = time.time()
    kl, illegal = store.surprise(net, link.DTYPES[dtype], n_test, count)
    seconds = time.time() - t0
    net.close()
    cand, counts, _, _ = store.ply_cum()
    rows = games[n_test:].astype(np.int64)
    lists = [cand[int(r[0]):int(r[0]) + int(c)] for r, c in zip(rows, counts[n_test:])]
    rows[:, 0] -= rows[0, 0]
    w = surprise_weights(kl, rows, lists, lam)
    picked = np.concatenate([r[0] + np.asarray(c, dtype=np.int64) for r, c in zip(rows, lists)])
    share = max((float(w[r[0] + np.asarray(c, dtype=np.int64)].max()) / len(c) for r, c in zip(rows, lists) if len(c)),
                default=0.0)
    k = kl[picked] if len(picked) else np.zeros(1)
    log("Policy surprise: %i games, %i plies in %.2f s against %s (%s); KL mean %.4f, median %.4f, max %.4f; the largest share "
        "one ply holds of its game: %.3f; %i targets that are no legal moves."
        % (count, len(kl), seconds, old_path, dtype, float(k.mean()), float(np.median(k)), float(k.max()), share, illegal))
    store.set_ply_weights(n_test, count, w)


# ---------------------------------------------------------------- reanalysis of stored plies

REANALYSE_SEED = 246813579            # train.py --reanalyse-fraction: the seed of the plan's own random.Random


def reanalyse_plan(games, ply_flags, candidates, candidate_count, blockers, first_game, n_games, fraction, slots, seed):
    """Which stored plies are searched again, and in which rounds -> [(wall mask, plies (n, 2) int32 of (game, ply))], n <= slots.
    From the store's mirrors (SampleStore.mirror, ply_cum, game_blockers), pure Python.  C = the candidate plies of the games
    [first_game, first_game + n_games) that are neither passes nor BAD; round(fraction * C) of them are picked without
    replacement with a random.Random(seed) of the plan's own — the global `random` is not touched, so the minibatch draws of a run
    do not move — sorted by (wall mask, game, ply) and cut into rounds of at most `slots` plies that never span two masks."""
    from . import link
    if not 0.0 <= fraction <= 1.0:
        raise ValueError("the reanalysed fraction must lie in [0, 1]")
    if slots < 1:
        raise ValueError("a round needs at least one slot")
    if not (0 <= first_game and 0 <= n_games and first_game + n_games <= len(games)):
        raise ValueError("games [%d, %d) of %d" % (first_game, first_game + n_games, len(games)))
    skip = link.SAMPLES_PLY_PASS | link.SAMPLES_PLY_BAD
    eligible = []
    for g in range(first_game, first_game + n_games):
        first = int(games[g][0])
        for k in range(int(candidate_count[g])):
            p = int(candidates[first + k])
            if not int(ply_flags[first + p]) & skip:
                eligible.append((int(blockers[g]), g, p))
    picked = sorted(random.Random(seed).sample(eligible, round(fraction * len(eligible))))
    rounds = []
    for mask, g, p in picked:
        if not rounds or rounds[-1][0] != mask or len(rounds[-1][1]) >= slots:
            rounds.append((mask, []))
        rounds[-1][1].append((g, p))
    return [(mask, np.asarray(rows, dtype=np.int32).reshape(-1, 2)) for mask, rows in rounds]


def reanalysis_config(slots, visits, mask, max_plies, seed=REANALYSE_SEED):
    """The engine a reanalysis round runs on: `slots` positions on the walls `mask`, a fresh tree per position, no root noise, and
    visits + 1 so that no move ever comes due — every root stops at `visits` visits below it and nothing is played."""
    from . import link, selfplay
    cfg = selfplay.make_config(slots, visits + 1, seed=seed, fen=selfplay.START_FEN_PLAIN, max_plies=max_plies,
                               dirichlet_weight=0.0, flags=link.FLAG_NO_REUSE)
    cfg.blockers = int(mask)                         # (the start position is never searched: every round loads its own)
    return cfg


def _flat_targets(start, index, weight):
    """The targets of n plies (a read_plies result) as one float64 array [n * 833], equal cells of a ply added up."""
    n, cells = len(start) - 1, BOARD * BOARD * MOVE_TYPES
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(start)) * cells + index.astype(np.int64)
    return np.bincount(keys, weights=weight.astype(np.float64), minlength=n * cells)


def target_kl(old, new):
    """KL(old target || new target) per ply in float64, from two read_plies results (start, index, weight) of the same plies; a
    cell the new target lacks counts with a weight of 1e-12."""
    p, q = _flat_targets(*old), _flat_targets(*new)
    at = np.flatnonzero(p > 0.0)
    terms = p[at] * (np.log(p[at]) - np.log(np.maximum(q[at], 1e-12)))
    return np.bincount(at // (BOARD * BOARD * MOVE_TYPES), weights=terms, minlength=len(old[0]) - 1)


def reanalyse(store, net, dtype, plan, visits, slots, log=print, seed=REANALYSE_SEED):
    """Searches the plies of `plan` (reanalyse_plan) afresh with `net`, a link.Net, in `dtype` and makes the roots their policy
    targets and values, one wall mask after the other.  Per mask one engine of `slots` slots with a fresh tree per position, no
    root noise and visits + 1 so that no move ever comes due; per round: read_plies, set_positions (x | (ply & 1) << 63, o, the
    stored ply number; a short round padded with its first position), run(net, 1 + visits), root_report_device into a tensor
    allocated once, retarget on the round's records.  -> {"changed", "unchanged", "rounds", "seconds", "positions_per_second",
    "mean_kl" (KL(old target || new target) over the changed plies), "stage_seconds" (per stage, summed over the rounds)}."""
    import time
    from . import link
    if visits < 1:
        raise ValueError("a reanalysis search needs at least one visit")
    games, _ = store.mirror()
    max_plies = int(games[:, 1].max()) + 1 if len(games) else 1
    reports = torch.zeros(slots * link.ROOT_REPORT_WORDS, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stages = {k: 0.0 for k in ("read_plies", "set_positions", "run", "report", "retarget", "kl")}
    changed = unchanged = 0
    kls = []
    engine, engine_mask = None, None
    t_start = time.time()

    def lap(name, t0):
        t1 = time.time()
        stages[name] += t1 - t0
        return t1

    try:
        for mask, plies in plan:
            n = len(plies)
            t = time.time()
            boards, _, _, start, index, weight = store.read_plies(plies)
            t = lap("read_plies", t)
            loaded = np.empty((slots, 2), dtype=np.uint64)
            loaded[:n, 0] = boards[:, 0] | ((plies[:, 1].astype(np.uint64) & np.uint64(1)) << np.uint64(63))
            loaded[:n, 1] = boards[:, 1]
            loaded[n:] = loaded[0]
            at = np.empty(slots, dtype=np.int32)
            at[:n] = plies[:, 1]
            at[n:] = at[0]
            if engine is None or engine_mask != mask:
                if engine is not None:
                    engine.close()
                engine, engine_mask = link.Engine(reanalysis_config(slots, visits, mask, max_plies, seed)), mask
                t = time.time()
            engine.set_positions(loaded, at)
            t = lap("set_positions", t)
            engine.run(net, 1 + visits, dtype)               # the roots' evaluation and `visits` steps
            engine.sync()
            t = lap("run", t)
            engine.root_report_device(reports, 0, n)
            t = lap("report", t)
            status = store.retarget(plies, reports, mask)
            t = lap("retarget", t)
            _, _, _, start2, index2, weight2 = store.read_plies(plies)
            kl = target_kl((start, index, weight), (start2, index2, weight2))
            kls.append(kl[status == 1])
            changed += int((status == 1).sum())
            unchanged += int((status != 1).sum())
            lap("kl", t)
    finally:
        if engine is not None:
            engine.close()
    seconds = time.time() - t_start
    kls = np.concatenate(kls) if kls else np.zeros(0)
    out = {"changed": changed, "unchanged": unchanged, "rounds": len(plan), "seconds": seconds,
           "positions_per_second": (changed + unchanged) / seconds if seconds > 0 else 0.0,
           "mean_kl": float(kls.mean()) if len(kls) else 0.0, "stage_seconds": stages}
    log("Reanalysis: %i plies changed, %i unchanged in %i rounds of at most %i slots at %i visits: %.2f s, %.0f positions/s; "
        "mean KL(old target || new target) %.4f over the changed plies."
        % (changed, unchanged, len(plan), slots, visits, seconds, out["positions_per_second"], out["mean_kl"]))
    return out


def _apply_reanalysis(store, old_path, fraction, visits, slots, dtype, n_test, log):
    """One reanalysis of the training games [n_test, games) with the net at old_path, before the first step."""
    from . import link
    games, flags = store.mirror()
    cand, counts, _, _ = store.ply_cum()
    plan = reanalyse_plan(games, flags, cand, counts, store.game_blockers(), n_test, len(games) - n_test, fraction, slots,
                          REANALYSE_SEED)
    cw, bnp = model.load_model(old_path)
    net = link.Net(cw, bnp)
    try:
        return reanalyse(store, net, link.DTYPES[dtype], plan, visits, slots, log)
    finally:
        net.close()


# ---------------------------------------------------------------- the network (model.py:38-101)

# ---------------------------------------------------------------- proven outcomes for stored plies

def prove_refusal(depth, nodes):
    """Why train.py --prove-depth D --prove-nodes N is refused, or None: the limits of the alpha-beta search, checked before
    anything touches the device."""
    from . import link
    if not 1 <= depth <= link.ALPHABETA_MAX_DEPTH:
        return "--prove-depth must be 1 .. %d" % link.ALPHABETA_MAX_DEPTH
    if nodes == 0 and depth > link.ALPHABETA_UNBOUNDED_DEPTH:
        return "--prove-nodes 0 (no limit) is accepted up to --prove-depth %d only" % link.ALPHABETA_UNBOUNDED_DEPTH
    if nodes != 0 and nodes < link.MAX_MOVES:
        return "--prove-nodes must be 0 (no limit) or at least %d" % link.MAX_MOVES
    return None


def _apply_proofs(store, depth, nodes, policy, n_test, log):
    """One proof pass over the training games [n_test, games), before the first step (SampleStore.prove)."""
    games, _ = store.mirror()
    s = store.prove(n_test, len(games) - n_test, depth, nodes, retarget_wins=policy)
    log("Proofs: %i proven wins, %i proven losses among %i plies searched to depth %i (%s); %i contradict their game's result; "
        "%i policy targets replaced" % (s["wins"], s["losses"], s["visited"], depth,
                                        "at most %i nodes each" % nodes if nodes else "no node limit", s["contradicted"],
                                        s["retargeted"]))
    return s


# ---------------------------------------------------------------- lambda-returns as value targets

def _log_value_lambda(lam, games, log):
    """games: (plies, carries values?) per training game."""
    valued = [n for n, has in games if has]
    log("Value targets: lambda-returns (L = %g) over %i plies of %i games; %i games without values keep z."
        % (lam, sum(valued), len(valued), len(games) - len(valued)))


def _apply_value_lambda(store, lam, n_test, log):
    """One returns pass over the training games [n_test, games), after reanalysis and the proof pass: it reads the values and the
    proofs they left (SampleStore.value_returns)."""
    from . import link
    games, _ = store.mirror()
    store.value_returns(n_test, len(games) - n_test, lam)
    _log_value_lambda(lam, [(int(n), bool(w & link.SAMPLES_GAME_HAS_VALUES)) for _, n, w, _ in games[n_test:].tolist()], log)


def aux_random_init(filters, seed=1):
    """Fresh weights of the auxiliary heads in torch's layouts, with model.random_init's distributions (truncated normal,
    stddev 0.2 * sqrt(2 / fan_in); bias 0.01), from numpy's PCG64(seed) alone."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def weights(shape, fan_in):
        return model._truncated_normal(rng, shape, 0.2 * (2.0 / fan_in) ** 0.5)

    return {"aux_conv": weights((2, filters, 1, 1), filters), "aux_fc_weight": weights((1, BOARD * BOARD), BOARD * BOARD),
            "aux_fc_bias": np.full((1,), 0.01, dtype=np.float32), "reply_conv": weights((MOVE_TYPES, filters, 1, 1), filters)}


def aux_sidecar(path):
    """Where the auxiliary heads of the network at `path` are kept: plain arrays, no pickle."""
    return path + ".aux.npz"


class Network(nn.Module):
    """model.Network in NCHW: tensors are [n][c][x][y] (the reference's [n][x][y][c] permuted)."""

    def __init__(self, blocks=12, filters=128, reference_bn_affine=False, aux_heads=False, aux_seed=1):
        """aux_heads: two heads that exist only while training (include/ataxxzero_hip.h, "Auxiliary targets") — a 1x1 conv
        filters -> 2 (channel 0 through tanh: the ownership; channel 1 flattened into Linear(49, 1): the score in units of 49
        stones) and a 1x1 conv filters -> 17 (the reply logits) — read by aux_forward and forward_all; forward, the state_dict
        of the rest and to_numpy are what they are without them.  Their weights come from numpy's PCG64(aux_seed), truncated normal as
        model.random_init; torch's global generator is left as it was."""
        super().__init__()
        self.blocks, self.filters, self.aux_heads = blocks, filters, bool(aux_heads)

        def conv(cin, cout, k):
            return nn.Conv2d(cin, cout, k, padding=k // 2, bias=False)

        def bn():
            # tf.layers.batch_normalization defaults: momentum 0.99 (torch: 1 - 0.99), epsilon 1e-3
            return nn.BatchNorm2d(filters, eps=model.BN_EPSILON, momentum=0.01, affine=reference_bn_affine)

        self.convs = nn.ModuleList([conv(4, filters, 3)] + [conv(filters, filters, 3) for _ in range(2 * blocks)])
        self.bns = nn.ModuleList([bn() for _ in range(2 * blocks + 1)])
        self.policy = conv(filters, MOVE_TYPES, 1)
        self.value_conv = conv(filters, 1, 1)
        self.fc = nn.Linear(BOARD * BOARD, 1)
        if self.aux_heads:
            with torch.random.fork_rng(devices=[]):                        # (the modules' own initialisation is thrown away)
                self.aux_conv = conv(filters, 2, 1)
                self.aux_fc = nn.Linear(BOARD * BOARD, 1)
                self.reply_conv = conv(filters, MOVE_TYPES, 1)
            self.load_aux_numpy(aux_random_init(filters, aux_seed))

    def _trunk(self, x):
        h = F.relu(self.bns[0](self.convs[0](x)))
        for b in range(self.blocks):
            t = F.relu(self.bns[1 + 2 * b](self.convs[1 + 2 * b](h)))
            t = self.bns[2 + 2 * b](self.convs[2 + 2 * b](t))
            h = F.relu(t + h)
        return h

    def _heads(self, x, h):
        policy = self.policy(h)                                            # [n][17][x][y]
        v = self.value_conv(h).reshape(x.shape[0], BOARD * BOARD)          # index x*7 + y, as tf.reshape of [n,x,y,1]
        value = torch.tanh(self.fc(v))
        return policy.permute(0, 2, 3, 1), value                           # policy back to [n][x][y][17]

    def _aux_heads(self, x, h):
        a = self.aux_conv(h)
        ownership = torch.tanh(a[:, 0])
        score = self.aux_fc(a[:, 1].reshape(x.shape[0], BOARD * BOARD))
        return ownership, score, self.reply_conv(h).permute(0, 2, 3, 1)

    def aux_forward(self, x):
        """-> (ownership [n][x][y] in (-1, 1), score [n][1] in units of 49 stones, reply logits [n][x][y][17]): a pass through
        the tower of its own."""
        return self._aux_heads(x, self._trunk(x))

    def forward_all(self, x):
        """-> forward(x) + aux_forward(x) from ONE pass through the tower: what a training step uses, so that the batch-norm
        statistics are updated once per step."""
        h = self._trunk(x)
        return self._heads(x, h) + self._aux_heads(x, h)

    def aux_to_numpy(self):
        """The heads' weights as plain arrays (the sidecar of train())."""
        return {"aux_conv": self.aux_conv.weight.detach().cpu().numpy().copy(),
                "aux_fc_weight": self.aux_fc.weight.detach().cpu().numpy().copy(),
                "aux_fc_bias": self.aux_fc.bias.detach().cpu().numpy().copy(),
                "reply_conv": self.reply_conv.weight.detach().cpu().numpy().copy()}

    def load_aux_numpy(self, arrays):
        """False, with nothing changed, when an array is missing or a shape does not fit."""
        mine = {"aux_conv": self.aux_conv.weight, "aux_fc_weight": self.aux_fc.weight, "aux_fc_bias": self.aux_fc.bias,
                "reply_conv": self.reply_conv.weight}
        if any(k not in arrays or tuple(np.asarray(arrays[k]).shape) != tuple(p.shape) for k, p in mine.items()):
            return False
        with torch.no_grad():
            for k, p in mine.items():
                p.copy_(torch.from_numpy(np.ascontiguousarray(arrays[k], dtype=np.float32)))
        return True

    def forward(self, x):
        return self._heads(x, self._trunk(x))

    # .npy layout <-> torch: conv HWIO (i, j, c, o) <-> OIHW with H = x (i), W = y (j)
    def load_numpy(self, conv_weights, bn_params):
        with torch.no_grad():
            convs = list(self.convs) + [self.policy, self.value_conv]
            for m, w in zip(convs, conv_weights[:len(convs)]):
                m.weight.copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(w, (3, 2, 0, 1)))))
            self.fc.weight.copy_(torch.from_numpy(np.asarray(conv_weights[-2]).reshape(1, BOARD * BOARD)))
            self.fc.bias.copy_(torch.from_numpy(np.asarray(conv_weights[-1]).reshape(1)))
            for i, m in enumerate(self.bns):
                m.running_mean.copy_(torch.from_numpy(np.asarray(bn_params[2 * i])))
                m.running_var.copy_(torch.from_numpy(np.asarray(bn_params[2 * i + 1])))

    def to_numpy(self):
        convs = list(self.convs) + [self.policy, self.value_conv]
        cw = [np.ascontiguousarray(np.transpose(m.weight.detach().cpu().numpy(), (2, 3, 1, 0))) for m in convs]
        cw.append(self.fc.weight.detach().cpu().numpy().reshape(BOARD * BOARD, 1).copy())
        cw.append(self.fc.bias.detach().cpu().numpy().reshape(1).copy())
        bn = []
        for m in self.bns:
            bn.append(m.running_mean.detach().cpu().numpy().copy())
            bn.append(m.running_var.detach().cpu().numpy().copy())
        return cw, bn


def link_outputs(store, n, device, aux=False):
    """The three tensors a store's kernel writes a minibatch of n samples into, on `device` (aux: the seven)."""
    if torch.device(device).type != "cuda":
        raise RuntimeError("device samples need a GPU: the gather has no CPU path")
    return store.aux_outputs(n, device) if aux else store.outputs(n, device)


def losses(net, features, policies, values):
    """model.py:81-93: (policy cross-entropy, value MSE, 1e-4 * sum(l2_loss(w)) over trainable variables)."""
    x = features.permute(0, 3, 1, 2)
    logits, v = net(x)
    n = features.shape[0]
    logp = F.log_softmax(logits.reshape(n, -1), dim=1)
    policy_loss = -(policies.reshape(n, -1) * logp).sum(dim=1).mean()
    value_loss = ((values - v) ** 2).mean()
    reg = 1e-4 * sum((p ** 2).sum() / 2 for p in net.parameters() if p.requires_grad)
    return policy_loss, value_loss, reg


def _aux_loss_terms(predictions, ownership, score, reply, aux_weight):
    own, sc, logits = predictions
    n = own.shape[0]
    w_final, w_reply = aux_weight[:, 0], aux_weight[:, 1]
    per_own = ((own - ownership) ** 2).reshape(n, -1).mean(dim=1)
    per_score = ((sc - score / float(BOARD * BOARD)) ** 2).reshape(n)
    per_reply = -(reply.reshape(n, -1) * F.log_softmax(logits.reshape(n, -1), dim=1)).sum(dim=1)
    d_final, d_reply = w_final.sum().clamp(min=1.0), w_reply.sum().clamp(min=1.0)
    return (w_final * per_own).sum() / d_final, (w_final * per_score).sum() / d_final, (w_reply * per_reply).sum() / d_reply


def aux_losses(net, features, ownership, score, reply, aux_weight):
    """The three auxiliary losses of a Network with aux_heads -> (ownership, score, reply) scalars: per sample the mean over
    the 49 cells of (tanh - target)^2, (prediction - score / 49)^2, and the softmax cross-entropy of the reply over the 833
    cells; each averaged over the samples that have the target, sum w_i L_i / max(1, sum w_i) with w = aux_weight[:, 0] for the
    first two and aux_weight[:, 1] for the reply.  A pass through the tower of its own (net.aux_forward): a training step
    uses all_losses."""
    return _aux_loss_terms(net.aux_forward(features.permute(0, 3, 1, 2)), ownership, score, reply, aux_weight)


def all_losses(net, features, policies, values, ownership, score, reply, aux_weight):
    """losses(...) + aux_losses(...) -> six scalars from one pass through the tower (net.forward_all)."""
    logits, v, *aux = net.forward_all(features.permute(0, 3, 1, 2))
    n = features.shape[0]
    logp = F.log_softmax(logits.reshape(n, -1), dim=1)
    policy_loss = -(policies.reshape(n, -1) * logp).sum(dim=1).mean()
    value_loss = ((values - v) ** 2).mean()
    reg = 1e-4 * sum((p ** 2).sum() / 2 for p in net.parameters() if p.requires_grad)
    return (policy_loss, value_loss, reg) + _aux_loss_terms(aux, ownership, score, reply, aux_weight)


def make_optimizer(net, learning_rate):
    """tf.train.MomentumOptimizer(learning_rate, 0.9) (model.py:99-100): v <- 0.9 v + g, w <- w - lr v."""
    return torch.optim.SGD(net.parameters(), lr=learning_rate, momentum=0.9)


def train_step(net, opt, batch, aux_loss_weights=None):
    """One optimisation step of a net that is in train() mode on one minibatch -> the loss terms, as tensors.  batch: the three
    tensors of losses; with aux_loss_weights = (ownership, score, reply) the seven of all_losses, the three auxiliary terms
    added with those weights — one pass through the tower for all five heads."""
    if aux_loss_weights is not None:
        w_own, w_score, w_reply = aux_loss_weights
        terms = pl, vl, reg, ol, sl, rl = all_losses(net, *batch)
        loss = pl + vl + reg + w_own * ol + w_score * sl + w_reply * rl
    else:
        terms = pl, vl, reg = losses(net, *batch)
        loss = pl + vl + reg
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    return terms


def train(games_paths, old_path, new_path, steps=1000, minibatch_size=512, learning_rate=0.001, blocks=12, filters=128,
          reference_bn_affine=False, device=None, log=print, value_blend=0.0, device_samples=False, device_draws=False,
          surprise_weight=0.0, surprise_dtype="bf16", aux_ownership=0.0, aux_score=0.0, aux_reply=0.0,
          reanalyse_fraction=0.0, reanalyse_visits=0, reanalyse_slots=4096, reanalyse_dtype="bf16", prove_depth=0,
          prove_nodes=0, prove_policy=False, value_lambda=None):
    """device_samples: the entries are put into a link.SampleStore once and every minibatch is written by its kernel into
    tensors allocated once (make_minibatch_device) — the same minibatches as without it, no per-step host-to-device copy of
    the batch; device_draws (implies device_samples): the kernel also draws the samples.  Both need a GPU.
    surprise_weight L > 0 (implies device_draws, needs old_path): a training game's plies are drawn in proportion to
    (1 - L) + L n KL_i / sum KL, KL_i the surprise of ply i's policy target to the net at old_path evaluated in surprise_dtype
    (surprise_weights); the validation games stay uniform.
    reanalyse_fraction F > 0 (implies device_samples, needs old_path): before the first step, and before the surprise pass, that
    share of the training games' candidate plies is searched again with the net at old_path — reanalyse_visits visits each,
    reanalyse_slots positions per round, the tower in reanalyse_dtype — and trained on with the new visit distribution and search
    value (reanalyse); the validation games stay as recorded.  F = 0: nothing is called, every byte of the run is what it was.
    prove_depth D > 0 (implies device_samples, needs no net): after reanalysis and before the surprise pass, the device's
    alpha-beta search of depth D (prove_nodes nodes at most per ply, 0: no limit, D <= 3) runs on the training games' eligible
    plies; a ply it proves won or lost trains the value head on that outcome instead of the game's result, and under
    prove_policy a ply proven won takes the winning move as its policy target (SampleStore.prove); the validation games stay
    as recorded.  D = 0: nothing is called, every byte of the run is what it was.
    value_lambda L in [0, 1] (not None; refused together with a non-zero value_blend): a training game that carries "values"
    trains the value head on its plies' TD(lambda) returns over the search values that follow, closed with the result
    (lambda_returns).  With a store the returns are computed on the device after reanalysis and the proof pass — they see the
    refreshed values and the proofs — and before the surprise pass (SampleStore.value_returns); without one each entry's are
    computed once on the host, the same bits.  The validation games stay as recorded.  None: nothing is called, every byte of
    the run is what it was."""
    if value_lambda is not None:
        why = value_lambda_refusal(value_lambda, value_blend)
        if why:
            raise ValueError(why)
        value_lambda = float(value_lambda)
    if prove_depth != 0 or prove_nodes != 0 or prove_policy:
        why = prove_refusal(prove_depth, prove_nodes) if prove_depth != 0 else "--prove-nodes and --prove-policy need --prove-depth"
        if why:
            raise ValueError(why)
        device_samples = True
    if reanalyse_fraction != 0.0:
        if not 0.0 < reanalyse_fraction <= 1.0:
            raise ValueError("--reanalyse-fraction must lie in [0, 1]")
        if reanalyse_visits < 1 or reanalyse_slots < 1:
            raise ValueError("--reanalyse-visits and --reanalyse-slots must be at least 1")
        if old_path is None:
            raise ValueError("--reanalyse-fraction needs --old-path: the stored plies are searched with that network")
        device_samples = True
    if surprise_weight != 0.0:
        if not 0.0 < surprise_weight <= 1.0:
            raise ValueError("--surprise-weight must lie in [0, 1]")
        if old_path is None:
            raise ValueError("--surprise-weight needs --old-path: the surprise is measured against that network")
        device_samples = device_draws = True
    if min(aux_ownership, aux_score, aux_reply) < 0.0:
        raise ValueError("the auxiliary loss weights must not be negative")
    aux = bool(aux_ownership or aux_score or aux_reply)                   # all zero: no head, no sidecar, the run as it was
    random.seed(123456789)                                                # train.py:103
    entries = load_entries(games_paths)
    ply_count = sum(len(e["moves"]) for e in entries)
    log("Found %i games with %i plies." % (len(entries), ply_count))
    if any("full" in e for e in entries):                                 # playout cap: only FULL plies are policy targets
        ply_count = sum(sum(1 for f in e["full"] if f) if "full" in e else len(e["moves"]) for e in entries)
        log("Playout cap: %i of them are training targets (fully searched)." % ply_count)
    test_entries, train_entries = entries[:10], entries[10:]
    device = device or torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if old_path is not None:
        log("Loading old model.")
        cw, bnp = model.load_model(old_path)
        blocks, filters = (len(cw) - 5) // 2, int(cw[0].shape[-1])
    else:
        log("WARNING: Not loading a previous model!")
        cw, bnp = model.random_init(blocks, filters, seed=random.randrange(1 << 30))
    if aux:                                                               # heads that exist only while training
        net = Network(blocks, filters, reference_bn_affine, aux_heads=True, aux_seed=AUX_SEED).to(device)
        sidecar = aux_sidecar(old_path) if old_path is not None else None
        if sidecar is not None and os.path.exists(sidecar):
            with np.load(sidecar, allow_pickle=False) as kept:
                loaded = net.load_aux_numpy(kept)
            log("Auxiliary heads: %s." % ("read from " + sidecar if loaded else
                                          sidecar + " does not fit this network; freshly initialised"))
        else:
            log("Auxiliary heads: freshly initialised.")
    else:
        net = Network(blocks, filters, reference_bn_affine).to(device)
    net.load_numpy(cw, bnp)
    opt = make_optimizer(net, learning_rate)

    def to_dev(batch):
        return tuple(torch.from_numpy(a).to(device) for a in batch)

    store = _fill_store(entries, log, aux, reanalyse_fraction, prove_policy=prove_policy) if device_samples or device_draws \
        else None
    if aux:
        if store is not None:
            with_owners = int(store.game_owners()[min(10, len(entries)):].any(axis=1).sum())
        else:
            with_owners = sum(_entry_owner_row(e) is not None for e in train_entries)
        log("Auxiliary targets: %i of %i training games have owners (a final position the rules adjudicate)."
            % (with_owners, len(train_entries)))
    if store is not None:                                                 # validation: games [0, 10); training: [10, n)
        draws = "device" if device_draws else "reference"
        n_test = min(10, len(entries))
        if len(entries) <= n_test:
            raise ValueError("device samples need more than %d games" % n_test)
        train_out = link_outputs(store, minibatch_size, device, aux)
        if reanalyse_fraction > 0.0:
            _apply_reanalysis(store, old_path, reanalyse_fraction, reanalyse_visits, reanalyse_slots, reanalyse_dtype, n_test, log)
        if prove_depth > 0:
            _apply_proofs(store, prove_depth, prove_nodes, prove_policy, n_test, log)
        if value_lambda is not None:
            _apply_value_lambda(store, value_lambda, n_test, log)
        if surprise_weight > 0.0:
            _apply_surprise(store, old_path, surprise_weight, surprise_dtype, n_test, log)

        def next_batch(step):
            return make_minibatch_device(store, n_test, len(entries) - n_test, minibatch_size, value_blend, train_out, draws,
                                         step=1 + step, aux=aux)

        def check_store():
            failed = store.status() if device_draws else 0
            if failed:
                raise RuntimeError("%d samples found no drawable ply in 64 attempts" % failed)
    else:
        if value_lambda is not None:
            _log_value_lambda(value_lambda, [(len(e["boards"]), "values" in e) for e in train_entries], log)

        def next_batch(step):
            return to_dev(make_minibatch(train_entries, minibatch_size, value_blend, aux, value_lambda))

        def check_store():
            pass

    random.seed(123456789)                                                # train.py:131
    if store is not None:
        val_set = make_minibatch_device(store, 0, n_test, 2048, value_blend, link_outputs(store, 2048, device, aux), draws,
                                        step=0, aux=aux)
    else:
        val_set = to_dev(make_minibatch(test_entries, 2048, value_blend, aux))
    log("")
    log("Model dimensions: %i filters, %i blocks, %i parameters." % (
        filters, blocks, sum(int(np.prod(a.shape)) for a in cw)))
    log("Have %i augmented samples, and sampling %i in total." % (ply_count * 8, steps * minibatch_size))
    log("=== BEGINNING TRAINING ===")
    for step_number in range(steps):
        if step_number % 100 == 0:
            net.eval()
            with torch.no_grad():
                tail = ""
                if aux:
                    pl, vl, _, ol, sl, rl = all_losses(net, *val_set)
                    tail = "  own: %.6f  score: %.6f  reply: %.6f" % (float(ol), float(sl), float(rl))
                else:
                    pl, vl, _ = losses(net, *val_set)
            log("Step: %4i -- loss: %.6f  (policy: %.6f  value: %.6f%s)" % (step_number, float(pl + vl), float(pl), float(vl), tail))
            check_store()
        net.train()
        train_step(net, opt, next_batch(step_number), (aux_ownership, aux_score, aux_reply) if aux else None)
    check_store()
    model.save_model(new_path, *net.to_numpy())
    log("\x1b[35mSaved model to:\x1b[0m %s" % new_path)
    if aux:
        with open(aux_sidecar(new_path), "wb") as f:                      # (np.savez would append ".npz" to a bare path)
            np.savez(f, **net.aux_to_numpy())
        log("Saved the auxiliary heads to: %s" % aux_sidecar(new_path))
    return net
