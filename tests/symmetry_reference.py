"""Random symmetry per evaluation (azh_engine_set_random_symmetry), restated in plain Python / numpy: the 8 dihedral
symmetries on cells, bitboards and moves, the game's key word on the oracle's Philox, the position hash that picks the
symmetry, and the permutation of the 833 policy indices that turns "logits of the image" into "logits of the position".

Symmetry s: bit 0 mirrors x, bit 1 mirrors y, bit 2 then transposes, on the cells (x, y) = (sq % 7, 6 - sq // 7)."""
import ctypes

import numpy as np

from oracle import oracle_lib as orc

STREAM_EVAL_SYMMETRY = 5
M32 = 0xFFFFFFFF
BOARD_MASK = (1 << 49) - 1
# (dx, dy) = to - from of the 16 jump layers, in layer order (the clone is layer 16)
LAYER_DELTAS = ([(-2, dy) for dy in range(-2, 3)] + [(dx, dy) for dx in (-1, 0, 1) for dy in (-2, 2)] +
                [(2, dy) for dy in range(-2, 3)])


def image_xy(s, x, y):
    if s & 1:
        x = 6 - x
    if s & 2:
        y = 6 - y
    return (y, x) if s & 4 else (x, y)


def image_cell(s, sq):
    x, y = image_xy(s, sq % 7, 6 - sq // 7)
    return x + 7 * (6 - y)


def board(s, bb):
    """T_s(bitboard): a stone at image_s(c) for every stone at c"""
    return sum(1 << image_cell(s, c) for c in range(49) if (int(bb) >> c) & 1)


def move(s, mv):
    """T_s(move), u16 from | to << 8: both squares by image_s; anything that is no board move as it is"""
    frm, to = mv & 0xFF, (mv >> 8) & 0xFF
    if frm >= 49 or to >= 49:
        return mv
    return image_cell(s, frm) | (image_cell(s, to) << 8)


def flat(x, y, layer):
    return 119 * x + 17 * y + layer


def policy_index(mv):
    """flat index 119 to_x + 17 to_y + layer of a move (the layer from to - from; a clone is layer 16)"""
    frm, to = mv & 0xFF, (mv >> 8) & 0xFF
    fx, fy, tx, ty = frm % 7, 6 - frm // 7, to % 7, 6 - to // 7
    return flat(tx, ty, 16 if frm == to else LAYER_DELTAS.index((tx - fx, ty - fy)))


def image_delta(s, dx, dy):
    """the linear part of image_s on a difference of cells"""
    if s & 1:
        dx = -dx
    if s & 2:
        dy = -dy
    return (dy, dx) if s & 4 else (dx, dy)


def perm(s):
    """(833,) int64: perm[flat(cell, layer)] = flat(T_s(cell, layer)) — the destination cell by image_s, a jump layer by the
    image of its (dx, dy), the clone layer as it is; defined for every index, real move or not"""
    out = np.zeros(833, dtype=np.int64)
    for x in range(7):
        for y in range(7):
            ix, iy = image_xy(s, x, y)
            for layer in range(17):
                il = 16 if layer == 16 else LAYER_DELTAS.index(image_delta(s, *LAYER_DELTAS[layer]))
                out[flat(x, y, layer)] = flat(ix, iy, il)
    return out


PERMS = [perm(s) for s in range(8)]


def logits_of_the_position(image_logits, s):
    """The logits an evaluator that saw T_s(position) gave, as logits of the position itself: entry i is the image's entry
    perm_s[i].  image_logits: (..., 833) or (..., 7, 7, 17); s: one symmetry, or one per row."""
    rows = np.asarray(image_logits, dtype=np.float32).reshape(-1, 833)
    ss = np.broadcast_to(np.asarray(s, dtype=np.int64).reshape(-1), (len(rows),))
    return np.stack([rows[i][PERMS[int(ss[i])]] for i in range(len(rows))]) if len(rows) else rows.copy()


_KEYS = {}


def key(seed, uid):
    """philox(k0, k1; uid, 0, STREAM_EVAL_SYMMETRY, 0).v[0], on the oracle's Philox"""
    if (seed, uid) not in _KEYS:
        out = (ctypes.c_uint32 * 4)()
        orc.lib().orc_probe_philox(seed, uid, 0, STREAM_EVAL_SYMMETRY, 0, out)
        _KEYS[(seed, uid)] = int(out[0])
    return _KEYS[(seed, uid)]


def symmetry_of_key(k, mover, opponent):
    """the hash of the key word and the UNTRANSFORMED leaf board, arithmetic mod 2^32"""
    mover, opponent = int(mover), int(opponent)
    a = k & M32
    for w in (mover & M32, mover >> 32, opponent & M32, opponent >> 32):
        a = ((a ^ w) * 0x9E3779B1) & M32
        a ^= a >> 15
    a = (a * 0x85EBCA77) & M32
    a ^= a >> 13
    return a >> 29


def eval_symmetry(seed, uid, mover, opponent):
    return symmetry_of_key(key(seed, uid), mover, opponent)
