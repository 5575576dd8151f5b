"""uai.find_path — the walk from the position a kept search tree is rooted at to the position the front-end is asked to
search — with the rules oracle as its move generator: every child and grandchild of fixture positions is found by the
first path in move order (engine.set_state's loops, engine.py:458-460), anything further away is not."""
import ctypes

from ataxxzero_amd import uai
from oracle import oracle_lib as orc
from tests.helpers import load_gz


def successors(position):
    x, o, turn = position
    p = orc.Pos()
    p.pieces[0], p.pieces[1], p.blockers, p.turn, p.ply = x, o, 0, turn, 0
    if orc.result(p) != 0:
        return []
    out = []
    for mv in orc.movegen(p):
        q = orc.Pos()
        ctypes.memmove(ctypes.byref(q), ctypes.byref(p), ctypes.sizeof(p))
        orc.lib().orc_makemove(ctypes.byref(q), int(mv) & 0xFF, int(mv) >> 8)
        out.append((int(mv), (int(q.pieces[0]), int(q.pieces[1]), int(q.turn))))
    return out


class Cached:
    def __init__(self):
        self.known, self.calls = {}, 0

    def __call__(self, position):
        self.calls += 1
        if position not in self.known:
            self.known[position] = successors(position)
        return self.known[position]


def fixture_roots(n):
    recs = load_gz("rules_noblock.json.gz")
    out = []
    for rec in recs[:: max(1, len(recs) // (4 * n))]:
        p = orc.pos_from_fen(rec["fen"])
        if orc.result(p) == 0 and 4 <= len(orc.movegen(p)) <= 45:
            out.append((int(p.pieces[0]), int(p.pieces[1]), int(p.turn)))
    assert len(out) >= n
    return out[:n]


def test_every_child_and_grandchild_is_found_by_the_first_path_in_move_order():
    transpositions = 0
    for root in fixture_roots(8):
        gen = Cached()
        first = {}   # position -> the path expected: shorter first, then (first move, second move) order
        for m1, child in gen(root):
            first.setdefault(child, [m1])
        for m1, child in gen(root):
            for m2, grandchild in gen(child):
                transpositions += grandchild in first and first[grandchild] != [m1, m2]
                first.setdefault(grandchild, [m1, m2])
        first[root] = []   # (never a child or grandchild of itself: stones are only ever added)
        assert len(first) > 20
        for target, want in first.items():
            assert uai.find_path(root, target, gen) == want, (root, target)
        # one ply only: the grandchildren are out of reach
        for target, want in first.items():
            assert uai.find_path(root, target, gen, max_plies=1) == (want if len(want) < 2 else None)
        # three plies away, and another fixture's position: None
        far = 0
        for _, child in gen(root)[:3]:
            for _, grandchild in gen(child)[:3]:
                for m3, third in gen(grandchild)[:3]:
                    if third not in first:
                        assert uai.find_path(root, third, gen) is None
                        path = uai.find_path(root, third, gen, max_plies=3)
                        assert path is not None and len(path) == 3
                        far += 1
        assert far > 0
    assert transpositions > 0   # two paths to one board did occur, and the first one in move order was taken


def test_unrelated_positions_and_finished_roots():
    roots = fixture_roots(8)
    gen = Cached()
    for a, b in zip(roots, roots[1:]):
        assert uai.find_path(a, b, gen) is None
        assert uai.find_path(a, a, gen) == []
    full = ((1 << 49) - 1 - 1, 1, 0)   # a full board: finished, no successors
    assert successors(full) == []
    assert uai.find_path(full, roots[0], gen) is None and uai.find_path(full, full, gen) == []
