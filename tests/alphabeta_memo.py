"""The definition of tests/alphabeta_reference.py once more, fast enough for depth 8 on small walled regions: the same
value(p, d), the same `best` as the first maximum in rr.legal_moves order, no pruning, so every value is exact by
construction.  It works on integer masks (own stones, the opponent's, walls) and remembers, per wall mask, every
(own, opp, turn, d) it has met with both its value and the plain negamax node count below it.  That count is additive,
nodes(p, d) = sum over the moves of 1 + nodes(child, d - 1), so it is the count alphabeta_reference.search reports and stays
the upper bound of a sound pruned search.  Nothing shared with ataxxzero_amd/csrc/; the ring tables are rules_reference's.
"""
from tests import rules_reference as rr

WIN = 1000
NO_MOVE = 0xFFFF
ALL = (1 << 49) - 1
NEAR = [sum(1 << s for s in rr.NEAR[sq]) for sq in range(49)]
FAR = [sum(1 << s for s in rr.FAR[sq]) for sq in range(49)]

_memo = {}  # wall mask -> {(own, opp, turn, d): (value, nodes)}


def forget(walls=None):
    """drop what is remembered for one wall mask, or for all of them"""
    if walls is None:
        _memo.clear()
    else:
        _memo.pop(walls, None)


def entries():
    return sum(len(m) for m in _memo.values())


def pop(v):
    return bin(v).count("1")


def children(own, opp, walls):
    """[(move, the mover's stones after it, the opponent's)] in rr.legal_moves order: jumps by (from, to), then clones by
    destination"""
    empty = ALL & ~(own | opp | walls)
    out = []
    m = own
    while m:
        low = m & -m
        m ^= low
        frm = low.bit_length() - 1
        t = FAR[frm] & empty
        while t:
            bit = t & -t
            t ^= bit
            to = bit.bit_length() - 1
            flip = opp & NEAR[to]
            out.append((frm | (to << 8), (own ^ low) | bit | flip, opp ^ flip))
    t = empty
    while t:
        bit = t & -t
        t ^= bit
        to = bit.bit_length() - 1
        if NEAR[to] & own:
            flip = opp & NEAR[to]
            out.append((to | (to << 8), own | bit | flip, opp ^ flip))
    return out


def result(own, opp, turn, walls):
    """rr.result on masks: 0 ongoing, 1 x wins, 2 o wins; stones first, then the pass, then the count, a tie to x"""
    x, o = (own, opp) if turn == 0 else (opp, own)
    if x == 0:
        return 2
    if o == 0:
        return 1
    empty = ALL & ~(own | opp | walls)
    if empty:
        m = own
        while m:
            low = m & -m
            m ^= low
            sq = low.bit_length() - 1
            if (NEAR[sq] | FAR[sq]) & empty:
                return 0
    # the board is full, or the side to move is stuck and the empty squares go to its opponent
    nx, no = pop(x), pop(o)
    if turn == 0:
        no += pop(empty)
    else:
        nx += pop(empty)
    return 2 if nx < no else 1


def terminal(res, turn, d):
    return WIN + d if res == turn + 1 else -(WIN + d)


def value(own, opp, turn, d, walls):
    """(value(p, d), plain negamax nodes below p) of the position with `own` to move"""
    memo = _memo.setdefault(walls, {})
    key = (own, opp, turn, d)
    hit = memo.get(key)
    if hit is not None:
        return hit
    res = result(own, opp, turn, walls)
    if res != 0:
        out = (terminal(res, turn, d), 0)
    elif d == 0:
        out = (pop(own) - pop(opp), 0)
    else:
        best, nodes = None, 0
        for _, mine, theirs in children(own, opp, walls):
            v, n = value(theirs, mine, 1 - turn, d - 1, walls)
            nodes += 1 + n
            if best is None or -v > best:
                best = -v
        out = (best, nodes)
    memo[key] = out
    return out


def search_masks(x, o, walls, turn, d):
    """alphabeta_reference.search on masks -> (best, value, nodes of this one iteration)"""
    own, opp = (x, o) if turn == 0 else (o, x)
    res = result(own, opp, turn, walls)
    if res != 0:
        return NO_MOVE, terminal(res, turn, d), 0
    assert d >= 1
    best_move, best, nodes = None, None, 0
    for move, mine, theirs in children(own, opp, walls):
        v, n = value(theirs, mine, 1 - turn, d - 1, walls)
        nodes += 1 + n
        if best is None or -v > best:  # strictly: the first move of the greatest value
            best_move, best = move, -v
    return best_move, best, nodes


def search(b, d):
    x, o, walls = b.masks()
    return search_masks(x, o, walls, b.turn, d)


def all_depths(b, depth):
    return [search(b, d) for d in range(1, depth + 1)]


# ---- beside the definition: what pruning is worth.  Not used for any value; its own value is held to the memo's.

INF = 1 << 20


def _pruned(own, opp, turn, rem, alpha, beta, walls, count):
    """fail-soft alpha-beta below an unfinished position with rem >= 1 plies left, moves in `children` order, the window
    handed down whole, (-beta, -max(alpha, best so far)); a position with one ply left is not pruned (its children are
    scored side by side), which is how include/ataxxzero_hip.h's search spends its last ply"""
    kids = children(own, opp, walls)
    if rem == 1:
        count[0] += len(kids)
        return max(-value(theirs, mine, 1 - turn, 0, walls)[0] for _, mine, theirs in kids)
    best = -INF
    for _, mine, theirs in kids:
        if alpha >= beta:
            break
        count[0] += 1
        res = result(theirs, mine, 1 - turn, walls)
        v = -terminal(res, 1 - turn, rem - 1) if res != 0 else -_pruned(theirs, mine, 1 - turn, rem - 1, -beta, -alpha, walls, count)
        best = max(best, v)
        alpha = max(alpha, v)
    return best


def pruned_nodes(b, d):
    """the nodes a textbook alpha-beta of iteration d enters below the unfinished root b, counted as the definition counts
    them: between the root's move count and the plain negamax count.  A search that hands a wider window down than it has enters
    more."""
    x, o, walls = b.masks()
    own, opp = (x, o) if b.turn == 0 else (o, x)
    count = [0]
    v = _pruned(own, opp, b.turn, d, -INF, INF, walls, count)
    assert v == search(b, d)[1]
    return count[0]
