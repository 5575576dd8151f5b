"""Random symmetry per evaluation, the parts that need no device: the library's host functions (azh_symmetry_board,
azh_symmetry_move, azh_eval_symmetry — the same functions the kernels call) against the trainer's symmetries, against the
restatement in tests/symmetry_reference.py, and the spread of the position hash over the 8 symmetries."""
import numpy as np

from ataxxzero_amd import link, training
from tests import symmetry_reference as sr

START_X = (1 << 42) | (1 << 6)        # x5o/7/7/7/7/7/o5x: x on a7 and g1, o on g7 and a1, x to move
START_O = (1 << 48) | (1 << 0)
SEEDS = (20260101, 0x1234567_89ABCDEF, 7)
UIDS = (0, 1, 0xFFFFFFFF)


def _plane(bb):
    """[x][y][1] stone plane of a bitboard, cells (x, y) = (sq % 7, 6 - sq // 7)"""
    arr = np.zeros((7, 7, 1), dtype=np.int8)
    for sq in range(49):
        if (bb >> sq) & 1:
            arr[sq % 7, 6 - sq // 7, 0] = 1
    return arr


def _bitboard(arr):
    return sum(1 << (x + 7 * (6 - y)) for x in range(7) for y in range(7) if arr[x, y, 0])


def _random_boards(rng, n):
    """n positions, each cell empty / mover / opponent with equal chance -> [(mover, opponent)]"""
    cells = rng.integers(0, 3, size=(n, 49))
    return [(sum(1 << c for c in range(49) if row[c] == 1), sum(1 << c for c in range(49) if row[c] == 2)) for row in cells]


def _move_value(mv):
    """u16 move -> the trainer's move value"""
    frm, to = mv & 0xFF, mv >> 8
    end = (to % 7, 6 - to // 7)
    return ("c", end) if frm == to else ((frm % 7, 6 - frm // 7), end)


def _all_moves():
    """every clone and every distance-2 jump of the empty-board geometry, u16"""
    out = [sq | (sq << 8) for sq in range(49)]
    for frm in range(49):
        for to in range(49):
            dx, dy = to % 7 - frm % 7, to // 7 - frm // 7
            if max(abs(dx), abs(dy)) == 2:
                out.append(frm | (to << 8))
    return out


def test_board_symmetry_is_the_trainers_on_the_stone_planes():
    rng = np.random.default_rng(11)
    boards = [int(v) & sr.BOARD_MASK for v in rng.integers(0, 1 << 62, size=200, dtype=np.uint64)] + [1 << c for c in range(49)]
    for s in range(8):
        for bb in boards:
            want = _bitboard(training.apply_symmetry(s, _plane(bb)))
            assert link.symmetry_board(s, bb) == want == sr.board(s, bb), (s, hex(bb))


def test_move_symmetry_is_the_trainers():
    moves = _all_moves()
    assert len(moves) == 49 + 480          # the 529 distinct moves of the board
    jumps = [m for m in moves if (m & 0xFF) != (m >> 8)]
    assert len({sr.policy_index(m) % 17 for m in jumps}) == 16
    for s in range(8):
        for mv in moves:
            got = link.symmetry_move(s, mv)
            assert _move_value(got) == training.apply_symmetry_to_move(s, _move_value(mv)), (s, mv)
            assert got == sr.move(s, mv)
            assert ((got & 0xFF) == (got >> 8)) == ((mv & 0xFF) == (mv >> 8))       # a clone stays a clone
    assert link.symmetry_move(3, 0xFFFF) == 0xFFFF                                   # a pass is no board move
    for bad in (-1, 8):
        try:
            link.symmetry_move(bad, 0)
        except link.AzhError:
            pass
        else:
            raise AssertionError("symmetry %d was accepted" % bad)


def test_policy_permutation_is_the_trainers_on_every_real_move():
    _, policy_to = training._symmetry_tables()
    real = sorted({sr.policy_index(m) for m in _all_moves()})
    assert len(real) == len(_all_moves())
    for s in range(8):
        p = sr.perm(s)
        assert sorted(p.tolist()) == list(range(833))                                # a permutation of all 833 indices
        assert (p[real] == policy_to[s][real]).all()
        for mv in _all_moves():
            assert p[sr.policy_index(mv)] == sr.policy_index(link.symmetry_move(s, mv))
        assert [link.symmetry_policy_index(s, i) for i in range(833)] == p.tolist()   # the library's, on all 833 indices
    for bad in ((8, 0), (0, 833), (-1, 0), (0, -1)):
        try:
            link.symmetry_policy_index(*bad)
        except link.AzhError:
            pass
        else:
            raise AssertionError("%r was accepted" % (bad,))
    # the wrapper: logits of the image -> logits of the position
    row = np.arange(833, dtype=np.float32)
    for s in range(8):
        assert (sr.logits_of_the_position(row, s)[0] == row[sr.perm(s)]).all()


def test_group_facts():
    rng = np.random.default_rng(5)
    boards = _random_boards(rng, 64)
    for m, o in boards:
        assert link.symmetry_board(0, m) == m
    for s in range(8):
        inverses = [t for t in range(8) if all(link.symmetry_board(t, link.symmetry_board(s, 1 << c)) == 1 << c for c in range(49))]
        assert len(inverses) == 1, (s, inverses)
        for m, o in boards:
            tm, to = link.symmetry_board(s, m), link.symmetry_board(s, o)
            assert link.symmetry_board(s, m | o) == tm | to
            assert tm & to == 0
            assert bin(tm).count("1") == bin(m).count("1") and bin(to).count("1") == bin(o).count("1")
            assert link.symmetry_board(inverses[0], tm) == m
    assert len({link.symmetry_board(s, 0b1011) for s in range(8)}) == 8              # the eight are distinct


def test_eval_symmetry_equals_the_restatement():
    rng = np.random.default_rng(23)
    boards = _random_boards(rng, 4096)
    for seed in SEEDS:
        for uid in UIDS:
            got = [link.eval_symmetry(seed, uid, m, o) for m, o in boards]
            assert got == [sr.eval_symmetry(seed, uid, m, o) for m, o in boards], (seed, uid)
            assert set(got) == set(range(8))
    # the seed's high half and the uid are part of the key
    assert len({sr.key(seed, uid) for seed in SEEDS + (SEEDS[0] ^ (1 << 40),) for uid in UIDS}) == 12


def _shares_ok(symmetries, what):
    counts = np.bincount(np.asarray(symmetries), minlength=8)
    share = counts / counts.sum()
    print(what, " ".join("%.3f" % v for v in share))
    assert len(counts) == 8 and share.min() >= 0.09 and share.max() <= 0.16, (what, share)


def test_every_symmetry_gets_its_share():
    """The spread condition: each symmetry's share in [9 %, 16 %] over random positions under three fixed keys, over the keys
    0..4095 at the start position, and over the 2401 boards "start position plus one stone each"."""
    rng = np.random.default_rng(31)
    boards = _random_boards(rng, 4096)
    plus_one = [(START_X | (1 << a), START_O | (1 << b)) for a in range(49) for b in range(49)]
    assert len(plus_one) == 2401
    for seed in SEEDS:                       # three fixed keys, through the library's own function
        _shares_ok([link.eval_symmetry(seed, 0, m, o) for m, o in boards], "random positions, seed %d" % seed)
        _shares_ok([link.eval_symmetry(seed, 0, m, o) for m, o in plus_one], "start plus one stone each, seed %d" % seed)
    # key words 0..4095 (the restated hash, equal to the library's by the test above), and the keys of the uids 0..4095
    _shares_ok([sr.symmetry_of_key(k, START_X, START_O) for k in range(4096)], "keys 0..4095 at the start position")
    _shares_ok([link.eval_symmetry(SEEDS[0], uid, START_X, START_O) for uid in range(4096)], "uids 0..4095 at the start position")
