"""The rules kernels on positions that random play from the start never reaches (tests/golden/rules_edge.json.gz, written by
the reference's Python rules: tests/golden/gen_rules_edge_fixtures.py): wave_movegen / make_move / the adjudication behind
azh_rules_batch, azh_makemove_batch, azh_features_batch, azh_perft, the engine's loaded roots, and the sampler of
azh_random_play.  Everything is exact: against the fixture, the C oracle and the cell-list restatement (tests/rules_reference.py)."""
import numpy as np
import pytest

from ataxxzero_amd import link
from oracle import oracle_lib as orc
from tests import rules_reference as rr
from tests.helpers import load_gz, synthetic_evals_distinct
from tests.helpers import BLOCK3_MASK, orc_pos, pocket_boards

pytestmark = pytest.mark.gpu

SETS = ["none", "block4", "block3", "wall8"]
_cache = {}


def edge_set(name):
    """-> (blockers mask, [record], [restated board], packed boards (n, 2) u64), computed once and left unchanged"""
    if name not in _cache:
        data = _cache.setdefault("data", None) or load_gz("rules_edge.json.gz")
        _cache["data"] = data
        mask = data["sets"][name]["mask"]
        recs = [r for r in data["positions"] if r["set"] == name]
        boards = [rr.Board.from_fen(r["fen"], mask) for r in recs]
        packed = np.array([b.packed() for b in boards], dtype=np.uint64)
        packed.setflags(write=False)
        _cache[name] = (mask, recs, boards, packed)
    return _cache[name]


def check_rows(boards, recs, moves, counts, results):
    for i, b in enumerate(boards):
        want = rr.legal_moves(b)
        assert results[i] == rr.result(b) == orc.result(orc_pos(b)), b.fen()
        if recs is not None:
            assert results[i] == recs[i]["result"], b.fen()
        assert counts[i] == rr.kernel_count(b), b.fen()
        assert (moves[i, counts[i]:] == 0).all(), b.fen()  # nothing is written past the count
        if b.count(rr.X) == 0 or b.count(rr.O) == 0:
            continue  # adjudicated before movegen: no move is listed
        assert moves[i, :counts[i]].tolist() == want == [int(m) for m in orc.movegen(orc_pos(b))], b.fen()  # exact order
        if recs is not None:
            assert (sorted(orc.move_string(m) for m in moves[i, :counts[i]]) or ["0000"]) == recs[i]["moves"]


@pytest.mark.parametrize("name", SETS)
def test_rules_batch_on_the_edge_positions(name):
    mask, recs, boards, packed = edge_set(name)
    moves, counts, results = link.rules_batch(packed, mask)
    assert moves.shape == (len(recs), link.MAX_MOVES) and counts.max() > 128
    check_rows(boards, recs, moves, counts, results)
    wide = int(np.argmax(counts))
    for sel in (slice(0, 1), slice(wide, wide + 1), slice(0, 63), slice(0, 64), slice(0, 65), slice(len(recs) - 65, len(recs))):
        m2, c2, r2 = link.rules_batch(packed[sel], mask)
        assert (m2 == moves[sel]).all() and (c2 == counts[sel]).all() and (r2 == results[sel]).all()


def test_rules_batch_follows_the_stones_first_order_where_the_reference_disagrees_with_itself():
    # the side to move is walled in and its opponent has no stones: no fixture (see gen_rules_edge_fixtures.py), the restatement
    for b, mask in pocket_boards():
        moves, counts, results = link.rules_batch(np.array([b.packed()], dtype=np.uint64), mask)
        check_rows([b], None, moves, counts, results)
        assert results[0] == 1 + b.turn and counts[0] == 0
    # boards on which one side has no stones, under every blocker set, restated only
    rng = np.random.default_rng(11)
    for name in SETS:
        mask = edge_set(name)[0]
        boards = []
        for k in range(24):
            cells = [rr.BLOCK if (mask >> sq) & 1 else (1 + k % 2 if rng.random() < (0.05, 0.4, 0.9)[k % 3] else rr.EMPTY)
                     for sq in range(49)]
            if cells.count(1 + k % 2):
                boards.append(rr.Board(cells, (k // 2) % 2))
        moves, counts, results = link.rules_batch(np.array([b.packed() for b in boards], dtype=np.uint64), mask)
        check_rows(boards, None, moves, counts, results)
        assert (counts == 0).all() and (results > 0).all()


@pytest.mark.parametrize("name", SETS)
def test_makemove_batch_on_every_recorded_successor(name):
    mask, recs, boards, packed = edge_set(name)
    rows, mvs, want = [], [], []
    for i, rec in enumerate(recs):
        for mv, fen2 in rec["succ"].items():
            rows.append(i)
            mvs.append(rr.move_from_string(mv))  # "0000" -> 0xFFFF, the pass
            want.append(rr.Board.from_fen(fen2, mask).packed())
    assert len(rows) > 5000 and mvs.count(rr.PASS) > 50
    out = link.makemove_batch(packed[rows], np.array(mvs, dtype=np.uint16))
    want = np.array(want, dtype=np.uint64)
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert len(bad) == 0, (recs[rows[bad[0]]]["fen"], rr.move_string(mvs[bad[0]]))
    # the restatement makes the same successors (flips included), so the three statements agree
    for j in range(0, len(rows), 37):
        assert rr.make_move(boards[rows[j]], mvs[j]).packed() == tuple(int(v) for v in want[j])


def test_features_batch_equals_the_restatement():
    def leaf(b):
        x, o, _ = b.masks()
        return (o, x) if b.turn else (x, o)

    for name in SETS:
        mask, _, boards, _ = edge_set(name)
        got = link.features_batch(np.array([leaf(b) for b in boards], dtype=np.uint64), mask)
        want = np.stack([rr.features(b) for b in boards])
        assert got.dtype == np.float32 and (got == want).all()
    rng = np.random.default_rng(20260318)
    for mask in rng.integers(0, 1 << 49, size=32, dtype=np.uint64):
        mask = int(mask)
        boards = []
        for k in range(9):
            d = (0.1, 0.5, 0.95)[k % 3]
            cells = [rr.BLOCK if (mask >> sq) & 1 else (int(rng.integers(1, 3)) if rng.random() < d else rr.EMPTY)
                     for sq in range(49)]
            boards.append(rr.Board(cells, k % 2))
        got = link.features_batch(np.array([leaf(b) for b in boards], dtype=np.uint64), mask)
        assert (got == np.stack([rr.features(b) for b in boards])).all()
        assert got[..., 3].sum() == 9 * bin(mask).count("1")


def test_perft_on_edge_positions_and_wide_roots():
    data = load_gz("rules_edge.json.gz")
    for ent in data["perft"]:
        mask = data["sets"][ent["set"]]["mask"]
        x, o, _ = rr.Board.from_fen(ent["fen"], mask).masks()
        turn = rr.Board.from_fen(ent["fen"], mask).turn
        for d, n in ent["depth"].items():
            assert link.perft(x, o, mask, turn, int(d)) == n, (ent["fen"], d)
    # six wide roots at depth 2, against the restatement: one thread of k_perft_level writes up to 193 children
    wide = []
    for name in ("none", "block3"):
        mask, recs, boards, _ = edge_set(name)
        order = sorted(range(len(recs)), key=lambda i: -rr.kernel_count(boards[i]))
        wide += [(boards[i], mask) for i in order[:3]]
    assert {b.turn for b, _ in wide} == {0, 1}
    for b, mask in wide:
        assert rr.count_moves(b) > 160
        x, o, _ = b.masks()
        assert link.perft(x, o, mask, b.turn, 1) == rr.count_moves(b)
        assert link.perft(x, o, mask, b.turn, 2) == rr.perft(b, 2), b.fen()
    # The widest boards leave the opponent a stone or two, so their depth-2 counts stay near 1,000, and no board met by a
    # hill climb on (moves of x) * (moves of o) has a depth-2 count above 8,400.  Two such boards, wide for both sides, go
    # one ply deeper: the frontier one root grows into passes 20,000 there.
    for fen, mask in (("oox1oo1/1ox1oxo/5o1/2x4/xxxxxxx/1oxo1xx/6o x", 0),
                      ("1ox1ooo/1xx2x1/1ox2-1/1xx2xx/2x2xo/1x-2x1/-xo2o1 x", BLOCK3_MASK)):
        b = rr.Board.from_fen(fen)
        x, o, bl = b.masks()
        assert bl == mask and rr.count_moves(b) > 128 and rr.perft(b, 2) > 6000
        want = rr.perft(b, 3)
        assert want > 20000
        assert link.perft(x, o, mask, b.turn, 2) == rr.perft(b, 2) and link.perft(x, o, mask, b.turn, 3) == want, fen


def edge_roots(name, limit=64):
    """ongoing edge positions for the engine: wide roots, one-stone roots, roots one ply from a full board or from a position
    whose side to move is stuck, then others"""
    mask, recs, boards, packed = edge_set(name)
    live = [i for i, b in enumerate(boards) if rr.result(b) == 0]
    ends_next = lambda b: any(rr.result(rr.make_move(b, m)) != 0 for m in rr.legal_moves(b))
    groups = [
        sorted((i for i in live if recs[i]["family"] == "wide"), key=lambda i: -rr.count_moves(boards[i])),
        [i for i in live if boards[i].count(rr.X) == 1 and boards[i].count(rr.O) == 1],
        [i for i in live if recs[i]["family"] == "near"],
        [i for i in live if recs[i]["family"] in ("random", "capture") and ends_next(boards[i])],
        [i for i in live if recs[i]["family"] == "random"],
    ]
    picked = []
    for grp, take in zip(groups, (12, 12, 12, 12, limit)):
        picked += [i for i in grp if i not in picked][:take]
    picked = picked[:limit]
    return mask, [recs[i] for i in picked], [boards[i] for i in picked], np.array(packed[picked])


@pytest.mark.parametrize("name", ["none", "block3", "wall8"])
def test_engine_on_edge_roots_matches_the_oracle_in_lock_step(name):
    from tests.engine_harness import compare_all, make_pair, run_lockstep

    mask, recs, boards, packed = edge_roots(name)
    G = len(boards)
    assert 32 <= G <= 64
    assert sum(rr.count_moves(b) > 128 for b in boards) >= (5 if name != "wall8" else 1)
    assert sum(b.count(rr.X) == 1 and b.count(rr.O) == 1 for b in boards) >= 8
    assert sum(r["family"] == "near" for r in recs) >= 8
    start = next(r["fen"] for r in edge_set(name)[1] if r["family"] == "few" and r["result"] == 0 and r["to_move"] == 1)
    oe, ge = make_pair(games=G, visits=32, seed=31, fen=start)
    assert oe.cfg.blockers == mask
    plies = np.zeros(G, dtype=np.int32)
    # a root on which a side has no stones is refused, cleanly: the error names the slot and the engine takes the next load
    bad = packed.copy()
    bad[G // 2, 1] = 0
    with pytest.raises(link.AzhError, match="slot %d" % (G // 2)):
        ge.set_positions(bad, plies)
    for e in (oe, ge):
        e.set_positions(packed, plies)
    for g in range(G):
        assert (ge.tree(g)[0][0] == packed[g]).all()
    compare_all(oe, ge, range(G))
    run_lockstep(oe, ge, 200, check_every=20, evaluator=synthetic_evals_distinct)
    compare_all(oe, ge, range(G))
    so, sg = oe.stats(), ge.stats()
    assert all(so[k] == sg[k] for k in so), (so, sg)
    assert so["plies"] >= G and so["games"] > 0  # moves were played from the loaded roots, and some games ended there


UNIFORM_ROOTS = [
    ("oxxxoxo/xoxxxxx/xoxxxxx/xxxxoxx/o1xxoox/xxxxxox/xxxxxxx o", 2),
    ("x5o/7/7/7/7/7/o5x x", 16),
    ("2oo1xx/o2o3/o2oooo/2oo2o/2oo3/o1oooo1/1o2o2 o", 157),
]
STREAM_RANDOM_PLAY = 2


def chi_square_p(observed, expected):
    from scipy import stats
    chi2 = float((((observed - expected) ** 2) / expected).sum())
    return chi2, float(stats.chi2.sf(chi2, len(observed) - 1))


@pytest.mark.parametrize("fen,M", UNIFORM_ROOTS)
def test_random_play_picks_its_first_move_uniformly(fen, M):
    """One ply from a root with M legal moves, 200 * M games, seeds 1, 2, 3 (fixed here, not chosen by looking at results): the
    histogram of the moves against the uniform one by a chi-square test, p > 1e-4.  Nine such histograms alarm falsely about
    once in a thousand, and with fixed seeds not at all once they have passed; a sampler that never picks one of 157 moves,
    or picks one of them twice as often, gives p far below 1e-20 at these counts."""
    b = rr.Board.from_fen(fen)
    legal = rr.legal_moves(b)
    assert len(legal) == M and rr.result(b) == 0
    x, o, _ = b.masks()
    n = 200 * M
    after = {m: rr.result(rr.make_move(b, m)) for m in legal}
    out = np.zeros(4, dtype=np.uint32)
    for seed in (1, 2, 3):
        plies, results, boards, moves = link.random_play(n, seed, x, o, 0, b.turn, max_plies=1)
        assert (plies == 1).all() and (boards[:, 0, 0] == x).all() and (boards[:, 0, 1] == o).all()
        played = moves[:, 0].astype(np.int64)
        hist = np.array([(played == m).sum() for m in legal])
        assert hist.sum() == n, "an illegal move was played"
        chi2, p = chi_square_p(hist, np.full(M, 200.0))
        print("M=%d seed=%d chi2=%.2f p=%.4g min=%d max=%d" % (M, seed, chi2, p, hist.min(), hist.max()))
        assert hist.min() > 0, "move %s never played" % rr.move_string(legal[int(hist.argmin())])
        assert p > 1e-4, (M, seed, chi2, p)
        assert (results == np.array([after[int(m)] for m in played])).all()  # the game is cut there and adjudicated
        # the draw itself, on the oracle's Philox: move number (r0 * M) >> 32 of game g at ply 0
        for g in range(0, n, max(1, n // 1500)):
            orc.lib().orc_probe_philox(seed, g, 0, STREAM_RANDOM_PLAY, 0, out.ctypes.data)
            assert played[g] == legal[(int(out[0]) * M) >> 32], (seed, g)


def test_random_play_picks_its_second_move_uniformly_given_the_first():
    b = rr.Board.from_fen("x5o/7/7/7/7/7/o5x x")
    x, o, _ = b.masks()
    firsts = rr.legal_moves(b)
    n = 200 * 16 * 16
    plies, results, boards, moves = link.random_play(n, 1, x, o, 0, 0, max_plies=2)
    assert (plies == 2).all()
    chi2, dof = 0.0, 0
    for f in firsts:
        sel = moves[:, 0] == f
        after = rr.make_move(b, f)
        assert (boards[sel, 1, 0] == after.masks()[0]).all() and (boards[sel, 1, 1] == after.masks()[1]).all()
        legal = rr.legal_moves(after)
        hist = np.array([(moves[sel, 1] == m).sum() for m in legal], dtype=np.float64)
        assert hist.sum() == sel.sum() > 100 * len(legal) and hist.min() > 0
        exp = hist.sum() / len(legal)
        chi2 += float(((hist - exp) ** 2 / exp).sum())
        dof += len(legal) - 1
    from scipy import stats
    p = float(stats.chi2.sf(chi2, dof))  # independent chi-squares given the first moves: their sum has the summed freedom
    print("ply 2: chi2=%.2f dof=%d p=%.4g" % (chi2, dof, p))
    assert p > 1e-4, (chi2, dof, p)
