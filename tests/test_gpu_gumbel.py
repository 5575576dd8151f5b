"""Gumbel root search with sequential halving on the MI355X (azh_engine_set_gumbel): the search in lock step with the numpy
restatement (tests/gumbel_reference.py) iteration by iteration — whole tree, root visits, the root's raw mark — the staged
records' moves and counts against gumbel_root, the game lines, wide roots, a root with one move, the device loop against
host stepping, off is off, set_visits while the mode is on, and the refusals."""
import json

import numpy as np
import pytest

from ataxxzero_amd import link
from oracle import oracle_lib as orc
from tests import engine_harness as eh
from tests import forced_reference as fr
from tests import gumbel_reference as gr
from tests import helpers
from tests import vl_reference as vlr
from tests.engine_harness import C_PUCT, SEED, WIDE_FEN_BIG, WIDE_FEN_MID

pytestmark = pytest.mark.gpu

C_VISIT, C_SCALE = 50.0, 1.0
ONE_MOVE_FEN = "oooxooo/oooxoxx/ooxxoxx/ooxxxxx/oooxxx1/oooxxxx/ooxxxxx o"
F32 = np.float32


def _expected_ply(tree, v0, g):
    """(move u16, {move: count}, unexpanded edges written) of the ply played from `tree`, by azh_gumbel_root — and the
    restatement agrees"""
    prior, W, n, moves, child = fr.root_arrays(tree)
    j, counts = link.gumbel_root(prior, W, n, v0, g, C_VISIT, C_SCALE)
    rj, rcounts = gr.root(prior, W, n, v0, g, C_VISIT, C_SCALE)
    assert j == rj and (counts == rcounts).all()
    assert int(n[j]) == int(n.max()) and counts.max() == 65535
    written = {int(mv): int(c) for mv, c in zip(moves, counts) if c != 0}
    return int(moves[j]), written, int(sum(1 for c, ch in zip(counts, child) if c != 0 and ch == vlr.NONE))


def _lock_step(e, visits, m, games, plies_checked=12, max_iterations=9000):
    """Slot 0 against the restatement, iteration by iteration, over the first `plies_checked` plies of `games` complete
    games (the later plies are played without the per-iteration comparison; every ply's record is checked) -> counters and
    the game lines."""
    seen = {"cv": set(), "schedule": set(), "differs": 0, "marks": 0, "mark_moves": 0, "unexpanded": 0, "plies": 0,
            "fallback": 0}
    root = {}        # (uid, ply) -> (a (M,) f32, g (M,) f32, v0)
    expected = {}    # (uid, ply) -> (move, {move: count})
    lines, done = [], 0
    for it in range(max_iterations):
        st = e.game_state(0)
        key = (st.uid, st.ply)
        b = None
        if st.phase == 1 and st.ply < plies_checked:
            pre = e.tree(0)
            mark = eh.root_mark(e)
            b = gr.select(pre, st.root_visits, visits, m, root[key][0], C_VISIT, C_SCALE, C_PUCT, False, 0)
        values = eh.step(e)[3]
        s2 = e.game_state(0)
        if st.phase == 0:
            # the root was evaluated: its noise and its own value
            assert (s2.uid, s2.ply, s2.phase) == (st.uid, st.ply, 1)
            prior = fr.root_arrays(e.tree(0))[0]
            g = link.gumbel_noise(SEED, st.uid, st.ply, len(prior))
            assert (g.view(np.uint32) == gr.noise(SEED, st.uid, st.ply, len(prior)).view(np.uint32)).all()
            root[key] = (gr.a_values(prior, g), g, F32(F32(values[0] + F32(1.0)) * F32(0.5)))
            M = len(prior)
            seen["schedule"] |= set(gr.seq(min(m, M), visits)) if st.ply < plies_checked else set()
        if b is not None:
            assert (s2.uid, s2.ply) == key
            post = e.tree(0)
            (eb, ei, ee, em), added = vlr.expected_tree(b, values, post)
            assert (eb == post[0]).all() and (ei == post[1]).all() and (ee == post[2]).all() and (em == post[3]).all(), it
            assert s2.root_visits == st.root_visits + added
            after = eh.root_mark(e)
            assert after == gr.next_mark(pre, mark, b.root_edge), (it, mark, b.root_edge, after)
            seen["cv"].add(b.cv)
            seen["fallback"] += int(b.gumbel is None)
            seen["differs"] += int(b.gumbel is not None and b.gumbel != b.puct)
            seen["marks"] += int(after is not None)
            seen["mark_moves"] += int(after != mark)
        if s2.phase == 2 and st.phase != 2:
            # the move of this ply is due: the next iteration plays it from this tree
            assert s2.root_visits == visits
            _, g, v0 = root[key]
            mv, written, unexpanded = _expected_ply(e.tree(0), v0, g)
            expected[key] = (mv, written)
            seen["unexpanded"] += unexpanded
        if s2.uid != st.uid:
            e.fetch()
            for slot, uid, result, kind, rows in eh.records3(e.staged_records()):
                assert kind & link.REC_KIND_GUMBEL and not kind & (link.REC_KIND_PLAYOUT_CAP | link.REC_KIND_FORCED)
                for ply, (move, w5, counts) in enumerate(rows):
                    assert (move, counts) == expected[(uid, ply)], (uid, ply)
                    seen["plies"] += 1
                done += 1
            lines += e.drain_json()
            if done >= games:
                break
    assert done >= games
    return seen, lines, expected


def _check_lines(lines, expected_by_game):
    """The game lines: the usual keys, every dists entry a distribution to 1e-6 whose values are c_j / sum(c) exactly"""
    assert len(lines) == len(expected_by_game) > 0
    for line, plies in zip(lines, expected_by_game):
        entry = json.loads(line)
        assert sorted(entry) == ["boards", "dists", "moves", "result"]
        assert len(entry["dists"]) == len(plies) == len(entry["moves"])
        for d, mv, (move, written) in zip(entry["dists"], entry["moves"], plies):
            total = sum(written.values())
            assert abs(sum(d.values()) - 1.0) < 1e-6
            assert d == {orc.move_string(k): float(c) / float(total) for k, c in written.items()}
            assert mv == orc.move_string(move)


@pytest.mark.parametrize("visits,m", [(16, 4), (33, 16)])
def test_lock_step_with_the_restatement(visits, m):
    e = eh.root_engine(1, visits, weight=0.0, flags=link.FLAG_NO_REUSE, gumbel=(m, C_VISIT, C_SCALE))
    seen, lines, expected = _lock_step(e, visits, m, 2)
    # every count the schedules of the checked plies hold was asked for (so every halving phase ran), the rule always found
    # its edge, and it did take edges PUCT would not have
    assert seen["cv"] == seen["schedule"] and len(seen["cv"]) >= 3 and seen["fallback"] == 0, seen
    assert seen["differs"] > 0 and seen["marks"] > 0 and seen["mark_moves"] > 0 and seen["unexpanded"] > 0, seen
    # (slot 0 plays the uids 0, 1, ... one after the other, and its lines come in that order)
    _check_lines(lines, [[expected[(uid, p)] for p in range(len(json.loads(l)["moves"]))] for uid, l in enumerate(lines)])
    assert seen["plies"] == sum(len(json.loads(l)["moves"]) for l in lines)
    e.close()


@pytest.mark.parametrize("fen,lo,hi,beyond", [(WIDE_FEN_MID, 65, 128, 64), (WIDE_FEN_BIG, 129, 256, 128)])
def test_wide_roots(fen, lo, hi, beyond):
    """One ply from a position with more than 64 and with more than 128 legal moves, every move considered (m = 256) and
    visits enough for two halving phases, in lock step with the restatement: candidates lie beyond a lane's first record."""
    p = orc.pos_from_fen(fen)
    M = len(orc.movegen(p))
    assert lo <= M <= hi
    visits, m = 160, 256
    e = eh.root_engine(1, visits, weight=0.0, flags=link.FLAG_NO_REUSE, gumbel=(m, C_VISIT, C_SCALE), edges_per_node=200)
    e.set_positions(np.array([[int(p.pieces[0]) | (int(p.turn) << 63), int(p.pieces[1])]], dtype=np.uint64),
                    np.zeros(1, dtype=np.int32))
    values = eh.step(e)[3]
    st = e.game_state(0)
    assert st.phase == 1
    prior = fr.root_arrays(e.tree(0))[0]
    assert len(prior) == M
    g = link.gumbel_noise(SEED, st.uid, st.ply, M)
    a, v0 = gr.a_values(prior, g), F32(F32(values[0] + F32(1.0)) * F32(0.5))
    high = differs = 0
    cvs = set()
    for it in range(visits):
        st = e.game_state(0)
        assert st.phase == 1 and st.root_visits == it
        pre, mark = e.tree(0), eh.root_mark(e)
        b = gr.select(pre, st.root_visits, visits, m, a, C_VISIT, C_SCALE, C_PUCT, False, 0)
        values = eh.step(e)[3]
        post = e.tree(0)
        (eb, ei, ee, em), added = vlr.expected_tree(b, values, post)
        assert (eb == post[0]).all() and (ei == post[1]).all() and (ee == post[2]).all() and (em == post[3]).all(), it
        assert eh.root_mark(e) == gr.next_mark(pre, mark, b.root_edge)
        assert b.gumbel is not None
        high += int(b.gumbel >= beyond)
        differs += int(b.gumbel != b.puct)
        cvs.add(b.cv)
    st = e.game_state(0)
    assert st.phase == 2 and st.root_visits == visits and high > 0 and differs > 0 and cvs == {0, 1}, (st.as_tuple(), high, cvs)
    mv, written, unexpanded = _expected_ply(e.tree(0), v0, g)
    assert unexpanded == 0 and len(written) >= 2     # (every move was considered and expanded: visits >= M)
    # the move is played from this tree (nothing is emitted: a loaded game writes no line)
    eh.step(e)
    s2 = e.game_state(0)
    assert s2.ply == 1 or s2.uid != st.uid
    e.close()


def test_a_root_with_one_legal_move():
    p = orc.pos_from_fen(ONE_MOVE_FEN)
    only = [int(x) for x in orc.movegen(p)]
    assert len(only) == 1 and orc.result(p) == 0
    visits = 6
    e = eh.root_engine(1, visits, weight=0.0, flags=link.FLAG_NO_REUSE, gumbel=(4, C_VISIT, C_SCALE))
    e.set_positions(np.array([[int(p.pieces[0]) | (int(p.turn) << 63), int(p.pieces[1])]], dtype=np.uint64),
                    np.zeros(1, dtype=np.int32))
    values = eh.step(e)[3]
    v0 = F32(F32(values[0] + F32(1.0)) * F32(0.5))
    prior = fr.root_arrays(e.tree(0))[0]
    g = link.gumbel_noise(SEED, 0, 0, 1)
    a = gr.a_values(prior, g)
    for it in range(visits):
        st = e.game_state(0)
        pre = e.tree(0)
        b = gr.select(pre, st.root_visits, visits, 4, a, C_VISIT, C_SCALE, C_PUCT, False, 0)
        assert b.gumbel == 0 and b.cv == it
        values = eh.step(e)[3]
        (eb, ei, ee, em), added = vlr.expected_tree(b, values, e.tree(0))
        post = e.tree(0)
        assert (eb == post[0]).all() and (ei == post[1]).all() and (ee == post[2]).all() and (em == post[3]).all()
    st = e.game_state(0)
    assert st.phase == 2 and st.root_visits == visits
    mv, written, _ = _expected_ply(e.tree(0), v0, g)
    assert mv == only[0] and written == {only[0]: 65535}
    # the next iteration plays it: the root is the position after the only move, one ply on
    eh.step(e)
    s2 = e.game_state(0)
    assert (s2.uid, s2.ply) == (0, 1)
    board = np.array([[int(p.pieces[0]) | (int(p.turn) << 63), int(p.pieces[1])]], dtype=np.uint64)
    assert (e.tree(0)[0][0] == link.makemove_batch(board, np.array(only, dtype=np.uint16))[0]).all()
    e.close()


@pytest.mark.parametrize("games,extras", [(5, False), (33, True), (130, False)])
def test_device_loop_equals_host_stepping(games, extras):
    net = eh.net()
    visits, m, n = 8, 4, 500
    a = eh.root_engine(games, visits, weight=0.0, flags=link.FLAG_NO_REUSE, gumbel=(m, C_VISIT, C_SCALE))
    b = eh.root_engine(games, visits, weight=0.0, flags=link.FLAG_NO_REUSE, gumbel=(m, C_VISIT, C_SCALE))
    if extras:
        for x in (a, b):
            x.set_random_symmetry(True)
            x.set_resign(0.0, 3, 0)     # values recorded, nobody resigns
    a.run(net, n, link.DTYPE_BF16)
    a.sync()
    for _ in range(n):
        b.select()
        b.eval(net, link.DTYPE_BF16)
        b.backup()
    eh.same(eh.dump(a), eh.dump(b))
    assert a.stats() == b.stats() and a.stats()["plies"] > 4 * games
    a.fetch(), b.fetch()
    ra, rb = eh.records3(a.staged_records()), eh.records3(b.staged_records())
    la, lb = a.drain_json(), b.drain_json()
    assert sorted(la) == sorted(lb) and len(ra) == len(rb) > 0
    for slot, uid, result, kind, rows in ra:
        assert kind & link.REC_KIND_GUMBEL and bool(kind & link.REC_KIND_VALUES) == extras
        for move, w5, counts in rows:
            assert max(counts.values()) == 65535 and min(counts.values()) >= 1
    for line in la:
        entry = json.loads(line)
        assert sorted(entry) == (["boards", "dists", "moves", "result", "values"] if extras else
                                 ["boards", "dists", "moves", "result"])
        for d in entry["dists"]:
            assert abs(sum(d.values()) - 1.0) < 1e-6
    a.close(), b.close()


def test_off_is_off():
    ref = eh.root_engine(3, 8, weight=0.0, flags=link.FLAG_NO_REUSE)
    never = eh.root_engine(3, 8, weight=0.0, flags=link.FLAG_NO_REUSE)
    off = eh.root_engine(3, 8, weight=0.0, flags=link.FLAG_NO_REUSE, gumbel=(4, C_VISIT, C_SCALE))
    off.set_gumbel(0)
    lines = {id(x): [] for x in (ref, never, off)}
    for it in range(1500):
        for x in (ref, never, off):
            eh.step(x)
        if it % 10 == 0 or len(lines[id(ref)]) >= 3:
            eh.same(eh.dump(ref), eh.dump(never))
            eh.same(eh.dump(ref), eh.dump(off))
        for x in (ref, never, off):
            x.fetch()
            for r in eh.records3(x.staged_records()):
                assert not r[3] & link.REC_KIND_GUMBEL
            lines[id(x)] += x.drain_json()
        if len(lines[id(ref)]) >= 3:
            break
    assert len(lines[id(ref)]) >= 3 and lines[id(ref)] == lines[id(never)] == lines[id(off)]
    assert ref.stats() == never.stats() == off.stats()
    # ... and the mode, switched on, does change the search (the comparison above is not vacuous)
    on = eh.root_engine(3, 8, weight=0.0, flags=link.FLAG_NO_REUSE, gumbel=(4, C_VISIT, C_SCALE))
    ref2 = eh.root_engine(3, 8, weight=0.0, flags=link.FLAG_NO_REUSE)
    differ = False
    for it in range(60):
        eh.step(on), eh.step(ref2)
        differ = differ or any((x.shape != y.shape or (x != y).any()) for g in range(3) for x, y in zip(on.tree(g), ref2.tree(g)))
    assert differ
    for x in (ref, never, off, on, ref2):
        x.close()


def test_set_visits_while_the_mode_is_on():
    """The engine's rows follow azh_engine_set_visits: a ply searched at the new threshold in lock step with the restatement
    on seq(r, new visits); a threshold whose table would be too large is refused and changes nothing."""
    e = eh.root_engine(1, 33, weight=0.0, flags=link.FLAG_NO_REUSE, gumbel=(4, C_VISIT, C_SCALE))
    e.set_visits(12)
    seen, lines, expected = _lock_step(e, 12, 4, 1, plies_checked=3)
    assert seen["cv"] == seen["schedule"] and len(seen["cv"]) >= 3 and seen["fallback"] == 0 and seen["differs"] > 0, seen
    e.close()
    big = eh.root_engine(1, 60000, weight=0.0, flags=link.FLAG_NO_REUSE, edges_per_node=8)
    with pytest.raises(link.AzhError):
        big.set_gumbel(256, C_VISIT, C_SCALE)          # 256 * 60000 entries
    big.set_visits(4096)
    big.set_gumbel(256, C_VISIT, C_SCALE)              # 2^20: the limit itself
    with pytest.raises(link.AzhError):
        big.set_visits(4097)
    big.set_visits(16)
    for _ in range(45):
        eh.step(big)
    assert big.stats()["plies"] >= 2
    big.set_gumbel(0)
    big.set_visits(60000)
    big.close()


def test_refusals_leave_the_engine_usable():
    e = eh.root_engine(4, 24, weight=0.0, flags=link.FLAG_NO_REUSE)
    for bad in ((-1, 50.0, 1.0), (257, 50.0, 1.0), (4, -1.0, 1.0), (4, float("nan"), 1.0), (4, float("inf"), 1.0),
                (4, 50.0, 0.0), (4, 50.0, -1.0), (4, 50.0, float("nan")), (4, 50.0, float("inf"))):
        with pytest.raises(link.AzhError):
            e.set_gumbel(*bad)
    eh.step(e)
    e.select()
    with pytest.raises(link.AzhError):
        e.set_gumbel(4)                        # a selected batch awaits its backup
    need, lb = e.leaves()
    e.set_evals(*helpers.synthetic_evals_distinct(lb))
    e.backup()
    temps = np.ones(400, dtype=np.float32)
    # each mode that is on refuses Gumbel; switched off again, Gumbel comes on and that mode's setter refuses in turn
    modes = [(lambda: e.set_playout_cap(6, 32768), lambda: e.set_playout_cap(0, 0)),
             (lambda: e.set_forced_playouts(2.0), lambda: e.set_forced_playouts(0.0)),
             (lambda: e.set_temperature(temps, None), lambda: e.set_temperature(None, None)),
             (lambda: e.set_temperature(None, temps), lambda: e.set_temperature(None, None)),
             (lambda: e.set_leaf_batch(4, 1), lambda: e.set_leaf_batch(1, 1)),
             (lambda: e.set_solver(True), lambda: e.set_solver(False))]
    for on, off in modes:
        on()
        with pytest.raises(link.AzhError):
            e.set_gumbel(4)
        off()
        e.set_gumbel(4)
        with pytest.raises(link.AzhError):
            on()
        off()                                  # switching a mode off is no request for it
        e.set_gumbel(0)
    e.set_gumbel(4)
    e.set_random_symmetry(True)                # allowed beside it
    e.set_resign(0.1, 3, 0)
    for _ in range(60):
        eh.step(e)
    assert e.stats()["plies"] > 0
    e.close()
    # the create-time requirements: a fresh root every ply, no Dirichlet mix, and none of the four flags
    for flags, weight in ((0, 0.0), (link.FLAG_NO_REUSE, 0.25),
                          (link.FLAG_NO_REUSE | link.FLAG_TWO_NETS, 0.0), (link.FLAG_NO_REUSE | link.FLAG_ONE_RANDOM_MOVE, 0.0),
                          (link.FLAG_NO_REUSE | link.FLAG_SAMPLE_POW5, 0.0), (link.FLAG_NO_REUSE | link.FLAG_EVAL_CACHE, 0.0)):
        r = eh.root_engine(4, 24, weight=weight, flags=flags)
        with pytest.raises(link.AzhError):
            r.set_gumbel(4)
        r.set_gumbel(0)                        # switching off is no request for the mode
        if not flags & link.FLAG_TWO_NETS:
            for _ in range(30):
                eh.step(r)
            assert r.stats()["steps"] > 0
        r.close()


def test_the_generator_with_gumbel_actions(tmp_path):
    """accelerated_generate_games.py --gumbel-actions M: the default cache is switched off with a note, the lines keep their
    keys, replay under the rules, and their dists are distributions over more moves than the ply had visits."""
    res, games_path = eh.generator(tmp_path, "--gumbel-actions", "4", "--gumbel-c-visit", "50", "--gumbel-c-scale", "1")
    text = res.stdout.decode()
    assert res.returncode == 0, text[-2000:] + res.stderr.decode()[-2000:]
    assert "Note: --gumbel-actions searches without the evaluation cache" in text
    lines = [l for l in open(games_path) if l.strip()]
    assert len(lines) == 20
    wide = 0
    for line in lines:
        entry = json.loads(line)
        assert list(entry) == ["boards", "dists", "moves", "result"]
        for d in entry["dists"]:
            assert abs(sum(d.values()) - 1.0) < 1e-6 and max(d.values()) > 0
            wide += int(len(d) > 6)
        bare = {k: v for k, v in entry.items() if k != "dists"}     # (the move played may have a count of 0: not in dists)
        assert helpers.replay_game_entry(bare, orc.START_FEN_SELFPLAY) == entry["result"]
    assert wide > 0
