"""A plain restatement of the Ataxx rules the kernels implement, on a 49-entry cell list: no bitboards, nothing shared with
oracle/ataxx_rules_oracle.c or ataxxzero_amd/csrc/azh_device.h.  The third, independent statement of the rules that the
tests set against the C oracle, the reference-written fixtures and the HIP kernels.

Square sq = file + 7 * rank (a1 = 0, g1 = 6, a7 = 42): the kernels' numbering.  A cell is EMPTY, X, O or BLOCK; `turn` is 0
when x is to move and 1 when o is.  A move is the kernels' 16-bit code from | to << 8, a clone has from == to (its destination),
PASS is 0xFFFF.

Adjudication follows the order the kernels document (the reference's C++ get_board_result): a side without stones loses
BEFORE the move list is looked at; only then a side to move that has no move hands every empty square to its opponent; a
full board goes to the larger count and an exact tie to x.  The reference's Python `result()` looks at the pass first; the
two orders differ on one kind of board (the side to move is stuck and its opponent has no stones), which DESIGN.md records.
"""
import random

import numpy as np

EMPTY, X, O, BLOCK = 0, 1, 2, 3
PASS = 0xFFFF
MAX_MOVES = 256  # AZH_MAX_MOVES: the width of every move list the kernels write


def _ring(sq, d):
    f, r = sq % 7, sq // 7
    return [ff + 7 * rr for rr in range(7) for ff in range(7) if max(abs(ff - f), abs(rr - r)) == d]


NEAR = [_ring(sq, 1) for sq in range(49)]  # ascending
FAR = [_ring(sq, 2) for sq in range(49)]   # ascending


class Board:
    def __init__(self, cells, turn):
        assert len(cells) == 49 and turn in (0, 1)
        self.cells = list(cells)
        self.turn = turn

    def copy(self):
        return Board(self.cells, self.turn)

    def count(self, v):
        return self.cells.count(v)

    # -- conversions (the only place a bit mask appears: the kernels' API speaks masks)
    @staticmethod
    def from_masks(x, o, blockers, turn):
        cells = []
        for sq in range(49):
            bit = 1 << sq
            n = (1 if x & bit else 0) + (1 if o & bit else 0) + (1 if blockers & bit else 0)
            assert n <= 1, "overlapping masks at square %d" % sq
            cells.append(X if x & bit else O if o & bit else BLOCK if blockers & bit else EMPTY)
        return Board(cells, turn)

    def masks(self):
        """(x, o, blockers) as 49-bit integers"""
        out = [0, 0, 0]
        for sq, v in enumerate(self.cells):
            if v != EMPTY:
                out[v - 1] |= 1 << sq
        return tuple(out)

    def packed(self):
        """(word0, word1) of the kernels' packed board: x | turn << 63, o"""
        x, o, _ = self.masks()
        return x | (self.turn << 63), o

    @staticmethod
    def from_fen(fen, blockers=0):
        """rows from rank 7 down to rank 1; 'x', 'o', '-' (blocker), digits skip; `blockers`: a further mask of blocked squares"""
        rows, side = fen.split()[:2]
        cells = [EMPTY] * 49
        for i, row in enumerate(rows.split("/")):
            f = 0
            for c in row:
                if c.isdigit():
                    f += int(c)
                    continue
                cells[f + 7 * (6 - i)] = {"x": X, "o": O, "-": BLOCK}[c.lower()]
                f += 1
            assert f == 7, fen
        for sq in range(49):
            if (blockers >> sq) & 1:
                assert cells[sq] in (EMPTY, BLOCK), fen
                cells[sq] = BLOCK
        return Board(cells, {"x": 0, "o": 1}[side.lower()])

    def fen(self):
        rows = []
        for rank in range(6, -1, -1):
            s, run = "", 0
            for f in range(7):
                v = self.cells[f + 7 * rank]
                if v == EMPTY:
                    run += 1
                    continue
                if run:
                    s += str(run)
                    run = 0
                s += ".xo-"[v]
            rows.append(s + (str(run) if run else ""))
        return "/".join(rows) + " " + "xo"[self.turn]

    def reference_cells(self):
        """the reference's board list: index x + 7 * y with y = 0 at rank 7; 1 = x, 2 = o, blockers and empties 0"""
        return [self.cells[x + 7 * (6 - y)] % 3 for y in range(7) for x in range(7)]


def mover(b):
    return X if b.turn == 0 else O


def legal_moves(b):
    """Every move in the kernels' order: jumps ascending by (from, to), then clones ascending by destination, a clone once
    per destination however many stones could make it.  Empty when the side to move must pass."""
    me = mover(b)
    jumps = [frm | (to << 8) for frm in range(49) if b.cells[frm] == me for to in FAR[frm] if b.cells[to] == EMPTY]
    clones = [to | (to << 8) for to in range(49)
              if b.cells[to] == EMPTY and any(b.cells[n] == me for n in NEAR[to])]
    return jumps + clones


def count_moves(b):
    return len(legal_moves(b))


def make_move(b, move):
    """the position after `move` (PASS only hands the turn over); the stones next to the destination change sides"""
    out = b.copy()
    out.turn = 1 - b.turn
    if move == PASS:
        return out
    frm, to = move & 0xFF, move >> 8
    me = mover(b)
    assert b.cells[to] == EMPTY
    if frm != to:
        assert b.cells[frm] == me and to in FAR[frm]
        out.cells[frm] = EMPTY
    out.cells[to] = me
    for n in NEAR[to]:
        if out.cells[n] in (X, O):
            out.cells[n] = me
    return out


def result(b):
    """0 ongoing, 1 x wins, 2 o wins, in the kernels' order of checks"""
    nx, no = b.count(X), b.count(O)
    if nx == 0:
        return 2
    if no == 0:
        return 1
    empty = b.count(EMPTY)
    if not legal_moves(b):
        if b.turn == 0:
            no += empty
        else:
            nx += empty
        empty = 0
    if empty == 0:
        return 2 if nx < no else 1
    return 0


def kernel_count(b):
    """the count wave_movegen returns: a board on which a side has no stones is adjudicated before any move is listed"""
    if b.count(X) == 0 or b.count(O) == 0:
        return 0
    return count_moves(b)


def orders_disagree(b):
    """the one kind of board on which the reference's Python result() (pass first) and the kernels' order (stones first) can
    give different winners: the side to move is stuck and its opponent has no stones"""
    other = O if b.turn == 0 else X
    return b.count(other) == 0 and b.count(mover(b)) > 0 and not legal_moves(b)


def features(b):
    """(7, 7, 4) f32 indexed [x][y][plane], x = file, y = 6 - rank: ones, the mover's stones, the opponent's, blockers"""
    out = np.zeros((7, 7, 4), dtype=np.float32)
    me = mover(b)
    for sq, v in enumerate(b.cells):
        x, y = sq % 7, 6 - sq // 7
        out[x, y, 0] = 1.0
        if v == BLOCK:
            out[x, y, 3] = 1.0
        elif v == me:
            out[x, y, 1] = 1.0
        elif v != EMPTY:
            out[x, y, 2] = 1.0
    return out


def perft(b, depth):
    """leaves of the move tree `depth` plies down; a position without a move has exactly one child, the pass; nothing is
    adjudicated on the way (azh_perft, the reference's perft.py)"""
    if depth == 0:
        return 1
    moves = legal_moves(b) or [PASS]
    if depth == 1:
        return len(moves)
    return sum(perft(make_move(b, m), depth - 1) for m in moves)


def perft_has_pass(b, depth):
    """whether some position strictly inside the tree (or the root) has to pass"""
    if depth == 0:
        return False
    moves = legal_moves(b)
    if not moves:
        return True
    return depth > 1 and any(perft_has_pass(make_move(b, m), depth - 1) for m in moves)


def square_name(sq):
    return "abcdefg"[sq % 7] + str(sq // 7 + 1)


def move_string(move):
    if move == PASS:
        return "0000"
    frm, to = move & 0xFF, move >> 8
    return square_name(to) if frm == to else square_name(frm) + square_name(to)


def move_from_string(s):
    sq = lambda t: "abcdefg".index(t[0]) + 7 * (int(t[1]) - 1)
    if s == "0000":
        return PASS
    if len(s) == 2:
        return sq(s) | (sq(s) << 8)
    return sq(s[:2]) | (sq(s[2:]) << 8)


# ---------------------------------------------------------------- the widest move list

def hill_climb(seed, blockers=0, restarts=6, trail=None):
    """Single-cell hill climb for the board with the most legal moves, x to move: from a random board, change one playable cell
    to another of EMPTY / X / O whenever that lengthens the move list, until no single change does; `restarts` times from
    `random.Random(seed)`.  -> (most moves, its board).  `trail`, if a list, collects (count, board) of every board accepted on
    the way.  A local search: what it returns is the widest board it met, not a bound on all boards."""
    rng = random.Random(seed)
    playable = [sq for sq in range(49) if not (blockers >> sq) & 1]
    best_n, best = -1, None
    for _ in range(restarts):
        cells = [BLOCK if (blockers >> sq) & 1 else rng.choice((EMPTY, EMPTY, X, O)) for sq in range(49)]
        b = Board(cells, 0)
        n = count_moves(b)
        improved = True
        while improved:
            improved = False
            order = [(sq, v) for sq in playable for v in (EMPTY, X, O)]
            rng.shuffle(order)
            for sq, v in order:
                old = b.cells[sq]
                if v == old:
                    continue
                b.cells[sq] = v
                m = count_moves(b)
                if m > n:
                    n, improved = m, True
                    if trail is not None:
                        trail.append((n, b.copy()))
                else:
                    b.cells[sq] = old
        if n > best_n:
            best_n, best = n, b.copy()
    return best_n, best
