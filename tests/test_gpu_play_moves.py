"""Moves named by the host (azh_engine_play_moves) and the root report (azh_engine_root_report) on the MI355X:
the re-root of a host-named move against the reference's own MCTS.play (tests/golden/engine_reuse_search.json.gz),
the subtree property on 64 games at once — every expected value computed on the host from the tree read BEFORE the
move — refusals, a game whose own move was due, and the report against the host's reading of the whole tree."""
import ctypes
import json

import numpy as np
import pytest

from ataxxzero_amd import link, model
from oracle import oracle_lib as orc
from tests import engine_fixture_checks as fx
from tests.engine_fixture_checks import _reference_random_games
from tests.engine_harness import check_marks, step
from tests.helpers import synthetic_evals_distinct

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
G = 64
SESSION_FLAGS = link.FLAG_TIE_FIRST | link.FLAG_PY_POSTERIOR


# ------------------------------------------------------------------ 1. the reference's MCTS.play

def test_host_named_moves_equal_mcts_play():
    """All 16 four-ply sequences: per ply the search is stepped on the host until the root has the fixture's visits —
    in exactly the fixture's number of steps, i.e. with exactly the inherited visits the reference had — the tree is the
    reference's edge for edge, and the fixture's move is played by the host.  visits = 60000 never comes due, so the
    device samples nothing."""
    recs = fx.reuse_fixtures()
    assert len(recs) == 16
    finished = 0
    for rec in recs:
        ocfg = fx.reuse_config(rec)
        cfg = link.Config(**{n: getattr(ocfg, n) for n, _ in orc.Config._fields_})
        cfg.visits = 60000
        ge = link.Engine(cfg)
        for p, want in enumerate(rec["plies"]):
            steps = 0
            for _ in range(want["root_visits"] + 2):
                s = ge.game_state(0)
                if s.phase == 1 and s.root_visits >= want["root_visits"]:
                    break
                assert ge.select() <= 1
                root_eval = ge.game_state(0).leaf_kind == link.LEAF_ROOT
                logits, values = synthetic_evals_distinct(ge.leaves()[1])
                ge.set_evals(logits, values)
                ge.backup()
                steps += 0 if root_eval else 1
            s = ge.game_state(0)
            print("record", rec["fen"], "ply", p, "steps", steps, "want", want["steps"], "root", s.root_visits)
            assert s.root_visits == want["root_visits"] and steps == want["steps"], (p, steps, want["steps"])
            assert s.ply == p and s.phase == 1
            fx.check_edges(ge.tree(0), want["edges"])
            status = ge.play_moves([orc.move_from_string(want["move"])])
            last = p + 1 == len(rec["plies"])
            if last and rec["kept_edges"] == []:
                assert status[0] == link.PLAY_FINISHED
                finished += 1
            else:
                assert status[0] == link.PLAY_KEPT, (p, status)
        s = ge.game_state(0)
        assert s.ply == len(rec["plies"]) and s.root_visits == rec["kept_root_visits"]
        fx.check_edges(ge.tree(0), rec["kept_edges"])
        st = ge.stats()
        assert st["plies"] == 0 and st["reroot_nodes"] > len(rec["plies"])
        ge.close()
    assert finished == 2  # (the two records whose last move ends the game)


# ------------------------------------------------------------------ 2. / 4. subtree property, root report

def _pack(cells, ply):
    x = o = 0
    for idx, v in enumerate(cells):
        sq = (idx % 7) + 7 * (6 - idx // 7)
        if v == 1:
            x |= 1 << sq
        elif v == 2:
            o |= 1 << sq
    return (x | ((ply & 1) << 63), o)


def _positions():
    """64 distinct positions of the six committed random-play games: slot 0 the last position of a game together with
    the move that ends it, slot 1 the position with the most legal moves (more than 64), the rest spread over the games."""
    sq = lambda xy: xy[0] + 7 * (6 - xy[1])
    seen, pool, last = set(), [], None
    for line in _reference_random_games():
        entry = json.loads(line)
        for p, cells in enumerate(entry["boards"]):
            b = _pack(cells, p)
            if b not in seen:
                seen.add(b)
                pool.append(b)
        m = entry["moves"][-1]
        mv = sq(m[1]) | (sq(m[1]) << 8) if m[0] == "c" else sq(m[0]) | (sq(m[1]) << 8)
        last = last or (_pack(entry["boards"][-1], len(entry["boards"]) - 1), mv)
    counts = link.rules_batch(np.array(pool, dtype=np.uint64), 0)[1]
    widest = pool[int(np.argmax(counts))]
    assert counts.max() > 64
    rest = [b for b in pool if b not in (last[0], widest)]
    picks = [last[0], widest] + rest[3::max(1, (len(rest) - 3) // (G - 2))][:G - 2]
    assert len(picks) == G and len(set(picks)) == G
    return np.array(picks, dtype=np.uint64), last[1]


def _oracle_child(board, mv):
    """(packed board after the move, its moves in generation order, its result) by the rules oracle."""
    p = orc.Pos()
    p.pieces[0], p.pieces[1] = int(board[0]) & ~(1 << 63), int(board[1])
    p.blockers, p.turn, p.ply = 0, int(board[0]) >> 63, 0
    orc.lib().orc_makemove(ctypes.byref(p), int(mv) & 0xFF, int(mv) >> 8)
    res = orc.result(p)
    moves = [] if res != 0 else [int(m) for m in orc.movegen(p)]
    return (int(p.pieces[0]) | (p.turn << 63), int(p.pieces[1])), moves, res


def _expected_after(tree, j):
    """The tree azh_engine_play_moves must leave when root edge j of `tree` is played, from `tree` alone: the child's
    subtree renumbered breadth-first in (parent order, edge order), every node's edges at the running edge count; or a
    fresh one-node tree when the edge has no child."""
    boards, info, edges, moves = tree
    first = int(info[0, 0])
    c = int(edges[first + j, 3])
    if c == NONE:
        nb, nm, res = _oracle_child(boards[0], moves[first + j])
        e = np.zeros((len(nm), 4), dtype=np.uint32)
        e[:, 3] = NONE
        tv = np.float32(0.0)
        if res != 0:
            tv = np.float32(1.0 if res == 1 else -1.0)
            if nb[0] >> 63:
                tv = -tv
        i = np.array([[0, len(nm) | (res << 16), 0, int(np.array([tv]).view(np.uint32)[0]) if res else 0]], dtype=np.uint32)
        return np.array([nb], dtype=np.uint64), i, e, np.array(nm, dtype=np.uint16)
    order, new_edges, new_moves, new_info = [c], [], [], []
    k = 0
    while k < len(order):
        old = order[k]
        of, m = int(info[old, 0]), int(info[old, 1] & 0xFFFF)
        new_info.append([len(new_edges) if m else 0, int(info[old, 1]), 0, int(info[old, 3])])
        for e_idx in range(of, of + m):
            row = [int(v) for v in edges[e_idx]]
            if row[3] != NONE:
                order.append(row[3])
                row[3] = len(order) - 1
            new_edges.append(row)
            new_moves.append(int(moves[e_idx]))
        k += 1
    return (boards[order], np.array(new_info, dtype=np.uint32), np.array(new_edges, dtype=np.uint32).reshape(-1, 4),
            np.array(new_moves, dtype=np.uint16))


def _host_report(tree, root_visits):
    """What azh_engine_root_report must say, read off the whole tree: header, root rows, and the principal variation by
    the stated rule (most visits, the first edge on a tie; ends before an edge with 0 visits, into a finished position,
    at an edge without a child, after PV_MAX moves)."""
    boards, info, edges, moves = tree
    first, m, res = int(info[0, 0]), int(info[0, 1] & 0xFFFF), int(info[0, 1] >> 16)
    rows = edges[first:first + m]
    pv, node = [], 0
    while len(pv) < link.PV_MAX:
        nf, nm, nres = int(info[node, 0]), int(info[node, 1] & 0xFFFF), int(info[node, 1] >> 16)
        if nres != 0 or nm == 0:
            break
        n = edges[nf:nf + nm, 1]
        j = int(np.argmax(n))   # (the first maximum)
        if int(n[j]) == 0:
            break
        pv.append((int(moves[nf + j]), int(n[j])))
        if int(edges[nf + j, 3]) == NONE:
            break
        node = int(edges[nf + j, 3])
    return {"root_visits": root_visits, "result": res, "expanded": int((rows[:, 3] != NONE).sum()),
            "moves": moves[first:first + m].tolist(), "visits": rows[:, 1].tolist(), "scores": rows[:, 2].tolist(),
            "priors": rows[:, 0].tolist(), "pv": pv}


def _check_reports(reports, trees, states, boards_of):
    kinds = {"empty_pv": 0, "finished": 0, "wide": 0, "deep": 0}
    for g, (r, t, s) in enumerate(zip(reports, trees, states)):
        want = _host_report(t, s.root_visits)
        got = {"root_visits": r.root_visits, "result": r.result, "expanded": r.expanded, "moves": r.moves.tolist(),
               "visits": r.visits.tolist(), "scores": r.scores.view(np.uint32).tolist(),
               "priors": r.priors.view(np.uint32).tolist(), "pv": list(zip(r.pv.tolist(), r.pv_visits.tolist()))}
        assert got == want, (g, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
        assert r.root_visits == int(r.visits.sum())
        # the line is a legal sequence of moves from the root
        b = np.array(boards_of[g], dtype=np.uint64).reshape(1, 2)
        for mv in r.pv:
            legal, counts, results = link.rules_batch(b, 0)
            assert results[0] == 0 and int(mv) in legal[0, :counts[0]].tolist(), (g, int(mv))
            b = link.makemove_batch(b, np.array([mv], dtype=np.uint16))
        kinds["empty_pv"] += len(r.pv) == 0 and r.result == 0
        kinds["finished"] += r.result != 0
        kinds["wide"] += len(r.moves) > 64
        kinds["deep"] += len(r.pv) >= 3
    return kinds


_SCENARIOS = {}


def _scenario(name):
    """One engine of 64 loaded games: search, read every tree, one play_moves, read every tree again, search on.
    Everything the tests below look at is recorded here, once per configuration."""
    if name in _SCENARIOS:
        return _SCENARIOS[name]
    K, flags, iterations = {"k1": (1, 0, 300), "k1_cache": (1, link.FLAG_EVAL_CACHE, 300), "k8": (8, 0, 60)}[name]
    conv, bn = model.random_init(4, 64, seed=5)
    net = link.Net(conv, bn)
    positions, ending_move = _positions()
    p = orc.pos_from_fen(orc.START_FEN_PLAIN)
    cfg = link.Config(games=G, visits=2000, max_plies=400, edges_per_node=96, c_puct=1.0, dirichlet_alpha=0.15,
                      dirichlet_weight=0.0, start_turn=0, seed=17, start_x=int(p.pieces[0]), start_o=int(p.pieces[1]),
                      blockers=0, flags=SESSION_FLAGS | flags)
    e = link.Engine(cfg)
    e.set_positions(positions, np.full(G, 10, np.int32))
    if K > 1:
        e.set_leaf_batch(K, 2)
    e.run(net, iterations, link.DTYPE_F32)
    e.sync()
    sc = {"engine": e, "net": net, "positions": positions}
    sc["before"] = [e.tree(g) for g in range(G)]
    sc["raw_before"] = [e.tree_raw(g) for g in range(G)]
    sc["state_before"] = [e.game_state(g) for g in range(G)]
    sc["report_before"] = e.root_report()
    # the moves: root edge by index (None: no move, -1: a move that is not legal)
    choice, moves = [], np.full(G, link.NO_MOVE, dtype=np.uint16)
    for g in range(G):
        boards, info, edges, mv = sc["before"][g]
        first, m = int(info[0, 0]), int(info[0, 1] & 0xFFFF)
        root_moves = mv[first:first + m].tolist()
        expanded = [j for j in range(m) if int(edges[first + j, 3]) != NONE]
        closed = [j for j in range(m) if int(edges[first + j, 3]) == NONE]
        if g == 0:
            j = root_moves.index(ending_move)
        elif g == 7:
            j = -1
            moves[g] = next(s | (s << 8) for s in range(49) if (s | (s << 8)) not in root_moves)
        elif g % 8 == 6:
            j = None
        elif g % 8 == 5 and closed:
            j = closed[g % len(closed)]
        else:
            j = expanded[g % len(expanded)]
        if j is not None and j >= 0:
            moves[g] = root_moves[j]
        choice.append(j)
    sc["choice"], sc["moves"] = choice, moves
    plies_before = e.stats()["plies"]
    sc["status"] = e.play_moves(moves)
    sc["after"] = [e.tree(g) for g in range(G)]
    sc["raw_after"] = [e.tree_raw(g) for g in range(G)]
    sc["state_after"] = [e.game_state(g) for g in range(G)]
    sc["report_after"] = e.root_report()
    sc["plies_played_by_device"] = e.stats()["plies"] - plies_before
    e.run(net, 100, link.DTYPE_F32)
    e.sync()
    sc["later"] = [e.tree(g) for g in range(G)]
    sc["state_later"] = [e.game_state(g) for g in range(G)]
    _SCENARIOS[name] = sc
    return sc


@pytest.mark.parametrize("name", ["k1", "k1_cache", "k8"])
def test_played_child_becomes_the_root_with_its_subtree(name):
    sc = _scenario(name)
    seen = {link.PLAY_KEPT: 0, link.PLAY_FRESH: 0, link.PLAY_FINISHED: 0, link.PLAY_NONE: 0, link.PLAY_ILLEGAL: 0}
    for g in range(G):
        j, status = sc["choice"][g], int(sc["status"][g])
        s0, s1 = sc["state_before"][g], sc["state_after"][g]
        seen[status] += 1
        if j is None or j < 0:
            assert status == (link.PLAY_NONE if j is None else link.PLAY_ILLEGAL)
            assert s0.as_tuple() == s1.as_tuple()
            assert all(np.array_equal(a, b) for a, b in zip(sc["before"][g], sc["after"][g]))
            assert np.array_equal(sc["raw_before"][g], sc["raw_after"][g])
            continue
        want = _expected_after(sc["before"][g], j)
        got = sc["after"][g]
        first = int(sc["before"][g][1][0, 0])
        had_child = int(sc["before"][g][2][first + j, 3]) != NONE
        finished = int(want[1][0, 1] >> 16) != 0
        assert status == (link.PLAY_FINISHED if finished else link.PLAY_KEPT if had_child else link.PLAY_FRESH), (g, status)
        for a, b, what in zip(got, want, ("boards", "info", "edges", "moves")):
            assert a.shape == b.shape and np.array_equal(a, b), (g, what)
        wf, wm = int(want[1][0, 0]), int(want[1][0, 1] & 0xFFFF)
        assert (s1.n_nodes, s1.n_edges) == (len(want[0]), len(want[2]))
        assert s1.root_visits == int(want[2][wf:wf + wm, 1].sum())
        if not had_child:
            assert s1.n_nodes == 1 and s1.root_visits == 0
        assert (s1.ply, s1.arena, s1.uid) == (s0.ply + 1, 1 - s0.arena, s0.uid)
        assert (s1.phase, s1.leaf_kind, s1.path_len) == (3 if finished else 0, link.LEAF_NONE, 0)
    assert seen[link.PLAY_KEPT] > 40 and seen[link.PLAY_FINISHED] >= 1 and seen[link.PLAY_NONE] == 8
    assert seen[link.PLAY_ILLEGAL] == 1 and seen[link.PLAY_FRESH] >= 1, seen
    assert sc["plies_played_by_device"] == 0
    # the search goes on from the kept trees: bookkeeping identities and the descent's mark
    e = sc["engine"]
    for g in range(G):
        s = sc["state_later"][g]
        boards, info, edges, moves = sc["later"][g]
        first, m = int(info[0, 0]), int(info[0, 1] & 0xFFFF)
        assert int(edges[first:first + m, 1].sum()) == s.root_visits
        if sc["choice"][g] is not None and sc["choice"][g] >= 0 and s.phase != 3:
            assert s.root_visits > sc["state_after"][g].root_visits and s.ply == sc["state_after"][g].ply
        kids = edges[:, 3][edges[:, 3] != NONE]
        assert len(set(kids.tolist())) == len(kids) == s.n_nodes - 1
        for e_idx in np.nonzero(edges[:, 3] != NONE)[0]:
            c = int(edges[e_idx, 3])
            cf, cm, cres = int(info[c, 0]), int(info[c, 1] & 0xFFFF), int(info[c, 1] >> 16)
            if cres == 0 and cm > 0:
                assert int(edges[e_idx, 1]) == 1 + int(edges[cf:cf + cm, 1].sum()), (g, int(e_idx))
    check_marks(e, range(G))
    assert e.stats()["plies"] == 0   # 400 iterations never reach 2000 visits: the device has sampled nothing


def test_evaluation_cache_is_rebuilt_by_a_host_named_move():
    """Cache on and cache off hold identical trees before the move, after it, and after 100 more iterations (the table of
    the new arena was rebuilt from the kept nodes: a stale or empty table would change which leaves go to the net, not the
    trees — so the saved evaluations are checked too)."""
    a, b = _scenario("k1"), _scenario("k1_cache")
    for key in ("before", "after", "later"):
        for g in range(G):
            (ba, ia, ea, ma), (bb, ib, eb, mb) = a[key][g], b[key][g]
            # (an unfinished node's value word is the cache's own copy of its evaluation: the uncached search keeps none)
            assert np.array_equal(ba, bb) and np.array_equal(ea, eb) and np.array_equal(ma, mb), (key, g)
            assert np.array_equal(ia[:, :2], ib[:, :2]), (key, g)
    sa, sb = a["engine"].stats(), b["engine"].stats()
    assert sa["steps"] == sb["steps"] and sb["cache_hits"] > 0
    assert sa["nn_evals"] == sb["nn_evals"] + sb["cache_hits"]


@pytest.mark.parametrize("name", ["k1", "k8"])
def test_root_report_equals_the_hosts_reading_of_the_tree(name):
    sc = _scenario(name)
    before = _check_reports(sc["report_before"], sc["before"], sc["state_before"], sc["positions"])
    roots_after = [t[0][0] for t in sc["after"]]
    after = _check_reports(sc["report_after"], sc["after"], sc["state_after"], roots_after)
    print("reports", name, before, after)
    assert before["wide"] >= 1 and before["deep"] >= 32
    assert after["finished"] >= 1 and after["empty_pv"] >= 1 and after["deep"] >= 1
    # a part of the slots, and the report of a slot the engine has never searched
    e = sc["engine"]
    part = e.root_report(first=5, n=3)
    whole = e.root_report()
    for k in range(3):
        assert part[k].root_visits == whole[5 + k].root_visits and part[k].pv.tolist() == whole[5 + k].pv.tolist()
    with pytest.raises(link.AzhError):
        e.root_report(first=G - 1, n=2)


# ------------------------------------------------------------------ 3. refusals, a game whose own move is due

def _small_engine(games=4, visits=200, flags=SESSION_FLAGS):
    p = orc.pos_from_fen(orc.START_FEN_PLAIN)
    return link.Engine(link.Config(games=games, visits=visits, max_plies=400, edges_per_node=96, c_puct=1.0,
                                   dirichlet_alpha=0.15, dirichlet_weight=0.0, start_turn=0, seed=3,
                                   start_x=int(p.pieces[0]), start_o=int(p.pieces[1]), blockers=0, flags=flags))


def _snapshot(e):
    return [(e.game_state(g).as_tuple(), [a.tobytes() for a in e.tree(g)], e.tree_raw(g).tobytes()) for g in range(e.G)]


def test_refused_while_a_selected_batch_awaits_its_backup():
    e = _small_engine()
    for _ in range(6):
        step(e)
    mv = int(e.root_report()[0].moves[0])
    e.select()
    snap = _snapshot(e)
    with pytest.raises(link.AzhError):
        e.play_moves([mv] * 4)
    assert _snapshot(e) == snap
    logits, values = synthetic_evals_distinct(e.leaves()[1])
    e.set_evals(logits, values)
    e.backup()
    assert (e.play_moves([mv] * 4) > 0).all()
    e.close()


def test_idle_slots_answer_busy_and_two_net_engines_refuse():
    e = _small_engine()
    e.set_game_limit(2)   # slots 2 and 3 go idle
    assert [e.game_state(g).phase for g in range(4)] == [0, 0, 3, 3]
    snap = _snapshot(e)
    mv = int(e.root_report()[0].moves[0])
    status = e.play_moves([mv] * 4)
    # (a root nobody has searched has no child to keep)
    assert status.tolist() == [link.PLAY_FRESH, link.PLAY_FRESH, link.PLAY_BUSY, link.PLAY_BUSY]
    assert _snapshot(e)[2:] == snap[2:]
    assert [e.game_state(g).ply for g in range(4)] == [1, 1, 0, 0]
    e.close()
    arena = _small_engine(flags=link.FLAG_ARENA)
    snap = _snapshot(arena)
    with pytest.raises(link.AzhError):
        arena.play_moves([mv] * 4)
    assert _snapshot(arena) == snap
    arena.close()


def test_a_game_whose_own_move_is_due_is_taken_out_of_the_queue():
    """A leaf-parallel search (K = 8) run exactly to its target ends with the move due (phase 2) and queued.  The
    documented route: play_moves plays the host's move IN PLACE of the sampled one.  Afterwards the search goes on, the
    ply has risen by exactly one and the device has played no move of its own (AZH_STAT_PLIES)."""
    conv, bn = model.random_init(2, 64, seed=9)
    net = link.Net(conv, bn)
    e = _small_engine(games=3, visits=400)
    e.set_leaf_batch(8, 2)
    e.set_visits(40)
    for _ in range(40):   # (a batch is cut to the visits that are missing, so the target is met exactly)
        e.run(net, 1, link.DTYPE_F32)
        if e.game_state(0).phase == 2:
            break
    states = [e.game_state(g) for g in range(3)]
    assert [(s.phase, s.root_visits, s.ply) for s in states] == [(2, 40, 0)] * 3
    reports = e.root_report()
    moves = [int(r.pv[0]) for r in reports]
    moves[2] = link.NO_MOVE   # game 2 keeps its own move: the device samples it in the next run
    status = e.play_moves(moves)
    assert status.tolist() == [link.PLAY_KEPT, link.PLAY_KEPT, link.PLAY_NONE]
    inherited = [e.game_state(g).root_visits for g in range(3)]
    assert inherited[:2] == [int(r.pv_visits[0]) - 1 for r in reports[:2]] and inherited[2] == 40
    assert [e.game_state(g).phase for g in range(3)] == [0, 0, 2]
    e.set_visits(400)
    e.run(net, 1 + 4, link.DTYPE_F32)
    e.sync()
    states = [e.game_state(g) for g in range(3)]
    assert [(s.ply, s.phase) for s in states] == [(1, 1)] * 3
    for g in range(2):   # (4 batches of up to 8 paths; a path that collided is not a visit)
        assert inherited[g] < states[g].root_visits <= inherited[g] + 32
    assert e.stats()["plies"] == 1   # game 2's sampled move, and no other
    # the host's moves were the ones played
    for g in range(2):
        want = link.makemove_batch(np.array(link.pack_board(int(e.cfg.start_x), int(e.cfg.start_o), 0)).reshape(1, 2),
                                   np.array([moves[g]], dtype=np.uint16))[0]
        assert e.tree(g)[0][0].tolist() == want.tolist()
    e.close()
