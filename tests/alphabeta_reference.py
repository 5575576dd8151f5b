"""The definition of the alpha-beta search (include/ataxxzero_hip.h, "alpha-beta search") in plain Python over
tests/rules_reference.py: negamax without pruning, `best` as the first maximum.  Nothing shared with the kernels.

value(p, d), seen from the side to move:
  1. rr.result(p) != 0: +(WIN + d) when the side to move has won, -(WIN + d) otherwise;
  2. d == 0: stones of the side to move minus stones of the opponent;
  3. else the maximum over m in rr.legal_moves(p) of -value(rr.make_move(p, m), d - 1).
nodes: the positions value was entered on, the root excluded.
"""
from tests import rules_reference as rr

WIN = 1000
NO_MOVE = 0xFFFF


def terminal(result, turn, d):
    return WIN + d if result == turn + 1 else -(WIN + d)


def value(b, d, count=None):
    """value(b, d); count, a one-entry list, gains the nodes entered below b"""
    res = rr.result(b)
    if res != 0:
        return terminal(res, b.turn, d)
    if d == 0:
        diff = b.count(rr.X) - b.count(rr.O)
        return diff if b.turn == 0 else -diff
    moves = rr.legal_moves(b)
    assert moves, "a position that is not finished has a move: no pass occurs in the search"
    best = None
    for m in moves:
        if count is not None:
            count[0] += 1
        v = -value(rr.make_move(b, m), d - 1, count)
        if best is None or v > best:
            best = v
    return best


def search(b, d):
    """-> (best(b, d), value(b, d), nodes of this one iteration); a finished root: (0xFFFF, rule 1 with d, 0)"""
    res = rr.result(b)
    if res != 0:
        return NO_MOVE, terminal(res, b.turn, d), 0
    assert d >= 1
    count = [0]
    best_move, best = None, None
    for m in rr.legal_moves(b):
        count[0] += 1
        v = -value(rr.make_move(b, m), d - 1, count)
        if best is None or v > best:  # strictly: the first move of the greatest value
            best_move, best = m, v
    return best_move, best, count[0]


def all_depths(b, depth):
    """[search(b, d) for d = 1 .. depth]: a test picks the depth the device reports"""
    return [search(b, d) for d in range(1, depth + 1)]
