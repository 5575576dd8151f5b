"""A plain restatement of the auxiliary training targets (include/ataxxzero_hip.h, "Auxiliary targets") on top of
tests/rules_reference.py's cell lists: the owners of a game's final position, and a sample's ownership, score, reply and weights.
Nothing here is shared with ataxxzero_amd/csrc/azh_device.h, link.samples_final_owners or training.aux_targets: boards are cell
lists, a symmetry is three coordinate operations, a policy cell is looked up in a table written out below."""
import numpy as np

from tests import rules_reference as rr

F32 = np.float32
# the layer of a jump in the (7, 7, 17) heat map: the rank of (dx, dy) among the distance-2 offsets, dx-major; a clone is 16
JUMP_LAYER = {d: i for i, d in enumerate((dx, dy) for dx in range(-2, 3) for dy in range(-2, 3) if max(abs(dx), abs(dy)) == 2)}


class Refused(Exception):
    """The move is not legal there, or the final position is the one board the two orders of adjudication disagree on."""


def final_owners(board, move):
    """`move` (rules_reference's code, PASS included) played on the rules_reference board -> (x-owned mask, o-owned mask,
    result) of the position reached; (0, 0, 0) when the game goes on there.  Refused for an illegal move."""
    legal = rr.legal_moves(board)
    if move == rr.PASS:
        if legal:
            raise Refused("a pass with %d moves available" % len(legal))
    elif move not in legal:
        raise Refused("move %#x is not legal" % move)
    final = rr.make_move(board, move)
    if rr.orders_disagree(final) and final.count(rr.EMPTY):
        raise Refused("the mover is stuck and its opponent has no stones")
    result = rr.result(final)
    if result == 0:
        return 0, 0, 0
    nx, no = final.count(rr.X), final.count(rr.O)
    if nx == 0 or no == 0:
        heir = rr.X if no == 0 else rr.O
    else:
        heir = rr.O if final.turn == 0 else rr.X          # the mover is stuck: the side NOT to move
    own = {rr.X: 0, rr.O: 0}
    for sq, v in enumerate(final.cells):
        if v == rr.BLOCK:
            continue
        own[heir if v == rr.EMPTY else v] |= 1 << sq
    assert result == (2 if bin(own[rr.X]).count("1") < bin(own[rr.O]).count("1") else 1)
    return own[rr.X], own[rr.O], result


def _xy(mv):
    """A game line's move -> (from (x, y) or None for a clone, to (x, y)), y = 0 at rank 7; None for a pass."""
    if mv in ("pass", "0000"):
        return None
    if isinstance(mv, str):
        sq = [("abcdefg".index(mv[k]), 7 - int(mv[k + 1])) for k in range(0, len(mv), 2)]
        return (None, sq[0]) if len(sq) == 1 else (sq[0], sq[1])
    return (None if mv[0] == "c" else tuple(mv[0]), tuple(mv[1]))


def entry_board(entry, ply):
    """The rules_reference board of an entry's ply: cells from boards[ply] (index x + 7 y, y = 0 at rank 7), the walls from its
    "blockers" (the same index), x to move on even plies."""
    cells = [rr.EMPTY] * 49
    for c, v in enumerate(entry["boards"][ply]):
        cells[c % 7 + 7 * (6 - c // 7)] = v
    for c in entry.get("blockers", ()):
        assert cells[c % 7 + 7 * (6 - c // 7)] == rr.EMPTY
        cells[c % 7 + 7 * (6 - c // 7)] = rr.BLOCK
    return rr.Board(cells, ply % 2)


def move_code(mv):
    xy = _xy(mv)
    if xy is None:
        return rr.PASS
    to = xy[1][0] + 7 * (6 - xy[1][1])
    frm = to if xy[0] is None else xy[0][0] + 7 * (6 - xy[0][1])
    return frm | to << 8


def entry_owners(entry):
    """(x-owned, o-owned, result of the final position) of a game line."""
    last = len(entry["boards"]) - 1
    return final_owners(entry_board(entry, last), move_code(entry["moves"][last]))


def image(s, xy):
    """Where the cell (x, y) lies under symmetry s: bit 0 mirrors x, bit 1 mirrors y, bit 2 then transposes."""
    x, y = xy
    if s & 1:
        x = 6 - x
    if s & 2:
        y = 6 - y
    return (y, x) if s & 4 else (x, y)


def heat_map(entry, ply, s):
    """The policy target of a ply under symmetry s as a (7, 7, 17) f32 array, or None where the ply is nobody's target: a pass,
    or weights whose f32 sum is off from 1 by 1e-3 or more."""
    if entry["moves"][ply] == "pass":
        return None
    items = entry["dists"][ply].items() if "dists" in entry else [(entry["moves"][ply], 1)]
    heat = np.zeros((7, 7, 17), dtype=F32)
    for mv, w in items:
        frm, to = _xy(mv)
        tx, ty = image(s, to)
        if frm is None:
            layer = 16
        else:
            fx, fy = image(s, frm)
            layer = JUMP_LAYER[(tx - fx, ty - fy)]
        heat[tx, ty, layer] += w
    return heat if abs(1 - heat.sum()) < 1e-3 else None


def targets(entry, ply, s):
    """-> (ownership (7, 7), score (1,), reply (7, 7, 17), aux_weight (2,)) of the sample (entry, ply, s), f32."""
    own_x, own_o, _ = entry_owners(entry)
    mine, theirs = (own_x, own_o) if ply % 2 == 0 else (own_o, own_x)
    ownership = np.zeros((7, 7), dtype=F32)
    for sq in range(49):
        x, y = image(s, (sq % 7, 6 - sq // 7))
        ownership[x, y] = ((mine >> sq) & 1) - ((theirs >> sq) & 1)
    score = np.array([bin(mine).count("1") - bin(theirs).count("1")], dtype=F32)
    reply = None
    if ply + 1 < len(entry["boards"]) and ("full" not in entry or entry["full"][ply + 1]):
        reply = heat_map(entry, ply + 1, s)
    weight = np.array([1.0 if own_x | own_o else 0.0, 0.0 if reply is None else 1.0], dtype=F32)
    return ownership, score, np.zeros((7, 7, 17), dtype=F32) if reply is None else reply, weight


def batch(entries, draws):
    """The four auxiliary arrays for draws (game, ply, symmetry), sample by sample."""
    rows = [targets(entries[g], p, s) for g, p, s in draws]
    return tuple(np.stack([r[k] for r in rows]).astype(F32) for k in range(4))
