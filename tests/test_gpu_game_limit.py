"""azh_engine_set_game_limit together with azh_engine_set_positions (include/ataxxzero_hip.h): "uids 0 .. N - 1
are played and nothing else" for engines whose slots were LOADED.  Every case of the oracle's own tests
(tests/test_oracle_search.py) is repeated in lock step — state and arena words at sync points, lines, every counter — and its
expectation is stated on the HIP engine directly as well: two engines that are wrong in the same way still fail.  All
comparisons are of integers and bit patterns."""
import json

import numpy as np
import pytest

from ataxxzero_amd import link, model
from oracle import oracle_lib as orc
from tests.helpers import cohort_positions, replay_game_entry, synthetic_evals
from tests.engine_harness import _oracle_follow, compare_all, make_pair
from tests.limit_fixtures import LIMIT_CASES, LIMIT_PLIES, cells_of, free_run

pytestmark = pytest.mark.gpu

CASES = LIMIT_CASES + [(33, 17)]   # ... and a slot range that is no multiple of anything


def pair(G, flags=0, visits=4, fen=orc.START_FEN_SELFPLAY, weight=0.25):
    """(oracle, HIP engine) with the configuration of tests/test_oracle_search.limit_engine"""
    return make_pair(games=G, visits=visits, max_plies=LIMIT_PLIES, seed=11, flags=flags, fen=fen, weight=weight)


def gsnap(e, stats=True):
    """every slot's state words, tree arrays and raw edge records, and the counters"""
    slots = [(e.game_state(g).as_tuple(), [a.tobytes() for a in e.tree(g)], e.tree_raw(g).tobytes()) for g in range(e.G)]
    return (slots, e.stats()) if stats else slots


def phases(e):
    return [e.game_state(g).phase for g in range(e.G)]


def gstep(e):
    e.select()
    logits, values = synthetic_evals(e.leaves()[1])
    e.set_evals(logits, values)
    e.backup()


def drive(ge, oe=None, twins=(), iterations=None, check_every=13, max_iters=6000):
    """Host-stepped iterations of `ge` until every slot is idle (or `iterations` of them), with the oracle `oe` in lock step
    (leaf lists every iteration, every state and arena word every `check_every`-th and at the end, counters at the end) and
    the `twins` — further HIP engines that must stay `ge`'s equal word for word — stepped beside it.
    -> (oracle games, partial ones included; ge's lines; uids seen in a slot of ge that was not idle)"""
    G = ge.G
    o_games, g_lines, live = [], [], set()
    twin_lines = [[] for _ in twins]

    def check():
        if oe is not None:
            compare_all(oe, ge, range(G))
        snap = gsnap(ge)
        for t in twins:
            assert gsnap(t) == snap

    it = 0
    while iterations is None or it < iterations:
        states = [ge.game_state(g) for g in range(G)]
        live |= {s.uid for s in states if s.phase != 3}
        if iterations is None and all(s.phase == 3 for s in states):
            break
        assert it < max_iters, "slots still playing after %d iterations" % max_iters
        n_g = ge.select()
        need_g, lb_g = ge.leaves()
        if oe is not None:
            n_o, need_o = oe.select()
            lb_o = oe.leaf_boards()
            assert n_o == n_g and (need_o == need_g).all(), it
            assert (lb_o[need_o != 0] == lb_g[need_o != 0]).all(), it
            logits, values = synthetic_evals(lb_o)
            oe.backup(logits, values)
            o_games += oe.pop_games(partial=True)
        else:
            logits, values = synthetic_evals(lb_g)
        ge.set_evals(logits, values)
        ge.backup()
        g_lines += ge.drain_json()
        for t, out in zip(twins, twin_lines):
            gstep(t)
            out += t.drain_json()
        if it % check_every == 0:
            check()
        it += 1
    check()
    if oe is not None:
        so, sg = oe.stats(), ge.stats()
        for k in so:
            assert so[k] == sg[k], (k, so[k], sg[k])
    for out in twin_lines:
        assert out == g_lines
    return o_games, g_lines, live


def assert_lines_are_the_oracles_complete_games(g_lines, o_games):
    """a self-play engine writes no line for a game that began at a loaded position; the others are the oracle's records"""
    want = sorted(json.dumps(r["entry"], sort_keys=True) for r in o_games if not r["partial"])
    assert sorted(json.dumps(json.loads(l), sort_keys=True) for l in g_lines) == want


def assert_loaded_and_idle(e, g, boards, plies):
    s = e.game_state(g)
    assert (s.phase, s.uid, s.ply, s.n_nodes, s.root_visits, s.leaf_kind) == (3, g, plies[g], 1, 0, orc.LEAF_NONE), (g, s.as_tuple())
    assert (e.tree(g)[0][0] == boards[g]).all(), g


@pytest.mark.parametrize("G,N", CASES)
def test_limit_idles_loaded_slots_in_either_call_order_and_plays_the_cohort_alone(G, N):
    boards, plies = cohort_positions(G, N)
    free_games, free_end = free_run(G, N)        # precondition, on the CPU oracle without a limit: a stray would end first
    assert min(free_end[g] for g in range(N, G)) < max(free_end[g] for g in range(N))
    (oa, ga), (ob, gb) = pair(G), pair(G)
    for e in (oa, ga):
        e.set_positions(boards, plies)
        e.set_game_limit(N)
    for e in (ob, gb):
        e.set_game_limit(N)
        e.set_positions(boards, plies)
    assert gsnap(ga) == gsnap(gb)
    compare_all(oa, ga, range(G))
    compare_all(ob, gb, range(G))
    for g in range(G):
        if g >= N:
            assert_loaded_and_idle(ga, g, boards, plies)
        else:
            s = ga.game_state(g)
            assert (s.phase, s.uid, s.ply) == (0, g, plies[g]) and (ga.tree(g)[0][0] == boards[g]).all()
    o_games, g_lines, live = drive(ga, oa, twins=[gb])
    assert live == set(range(N))
    st = ga.stats()
    assert st["games"] + st["dropped"] == N and st["ring_overflow"] == 0 and g_lines == []
    assert {r["uid"]: r["entry"] for r in o_games} == {u: r["entry"] for u, r in free_games.items() if u < N}
    # idle for good: nothing is selected, no counter moves, the slots past the limit still hold what they were loaded with
    assert ga.select() == 0
    ga.set_evals(*synthetic_evals(ga.leaves()[1]))
    ga.backup()
    assert ga.stats() == st and ga.drain_json() == []
    for g in range(N, G):
        assert_loaded_and_idle(ga, g, boards, plies)


@pytest.mark.parametrize("G,N", CASES)
def test_limit_raised_before_any_step_equals_the_high_limit_from_the_start(G, N):
    boards, plies = cohort_positions(G, N)
    (oa, ga), (ob, gb) = pair(G), pair(G)
    for e in (oa, ga):
        e.set_positions(boards, plies)
        e.set_game_limit(N)
        e.set_game_limit(G)          # idled with their loaded games, and resumed before anything ran
    for e in (ob, gb):
        e.set_game_limit(G)
        e.set_positions(boards, plies)
    gc = pair(G)[1]
    gc.set_game_limit(N)
    gc.set_positions(boards, plies)   # (the other order of getting there)
    gc.set_game_limit(G)
    assert gsnap(ga) == gsnap(gb) == gsnap(gc)
    compare_all(ob, gb, range(G))
    for g in range(G):
        s = ga.game_state(g)
        assert (s.phase, s.uid, s.ply, s.n_nodes) == (0, g, plies[g], 1) and (ga.tree(g)[0][0] == boards[g]).all()
    o_games, g_lines, live = drive(ga, oa, twins=[gb, gc])
    assert live == set(range(G))
    st = ga.stats()
    assert st["games"] + st["dropped"] == G and g_lines == []
    free_games, _ = free_run(G, N)
    assert {r["uid"]: r["entry"] for r in o_games} == {u: r["entry"] for u, r in free_games.items()}


@pytest.mark.parametrize("G,N", CASES)
def test_limit_raised_after_the_cohort_resumes_loaded_games_and_starts_fresh_ones(G, N):
    boards, plies = cohort_positions(G, N)
    oe, ge = pair(G)
    for e in (oe, ge):
        e.set_game_limit(N)
        e.set_positions(boards, plies)
    drive(ge, oe)
    first = ge.stats()
    assert first["games"] + first["dropped"] == N
    # raised past the slot count: the slots idled with a loaded game resume it; slots 0 and 1, whose loaded games are over,
    # start their next game (uids G, G + 1) at the start position; every other slot stays idle
    for e in (oe, ge):
        e.set_game_limit(G + 2)
    compare_all(oe, ge, range(G))
    start = orc.pos_from_fen(orc.START_FEN_SELFPLAY)
    for g in range(G):
        s = ge.game_state(g)
        if g >= N:
            assert (s.phase, s.uid, s.ply, s.n_nodes, s.root_visits) == (0, g, plies[g], 1, 0), (g, s.as_tuple())
            assert (ge.tree(g)[0][0] == boards[g]).all()
        elif g < 2:
            assert (s.phase, s.uid, s.ply, s.n_nodes, s.root_visits) == (0, G + g, 0, 1, 0), (g, s.as_tuple())
            assert [int(v) for v in ge.tree(g)[0][0]] == [int(start.pieces[0]) | (start.turn << 63), int(start.pieces[1])]
        else:
            assert (s.phase, s.uid) == (3, G + g)
    assert ge.stats() == first
    o_games, g_lines, live = drive(ge, oe)
    assert live == set(range(N, G)) | {G, G + 1}
    st = ge.stats()
    assert st["games"] + st["dropped"] == G + 2
    assert_lines_are_the_oracles_complete_games(g_lines, o_games)
    free_games, _ = free_run(G, N)
    assert sorted(r["uid"] for r in o_games if r["partial"]) == sorted(u for u in free_games if u >= N)
    for rec in o_games:
        if rec["partial"]:   # the game it was loaded with, from the loaded ply on: the game that uid is without a limit
            assert rec["entry"]["boards"][0] == cells_of(boards[rec["uid"]]) and rec["entry"] == free_games[rec["uid"]]["entry"]
    for line in g_lines:     # the fresh ones: whole games from the start position
        entry = json.loads(line)
        assert replay_game_entry(entry, orc.START_FEN_SELFPLAY) == entry["result"]
    assert len(g_lines) == st["games"] - first["games"] - sum(r["partial"] for r in o_games)


@pytest.mark.parametrize("G,N", CASES)
def test_limit_never_stops_a_loaded_game_whose_root_has_been_evaluated(G, N):
    boards, plies = cohort_positions(G, N)
    oe, ge = pair(G)
    twin = pair(G)[1]
    for e in (oe, ge, twin):
        e.set_positions(boards, plies)
    drive(ge, oe, twins=[twin], iterations=1)
    before = gsnap(ge)
    for e in (oe, ge):
        e.set_game_limit(N)
    assert gsnap(ge) == before == gsnap(twin)      # begun: the root evaluation is done, nothing is idled
    assert 3 not in phases(ge)
    o_games, g_lines, live = drive(ge, oe)
    assert live == set(range(G))
    st = ge.stats()
    assert st["games"] + st["dropped"] == G and g_lines == []
    free_games, _ = free_run(G, N)
    assert {r["uid"]: r["entry"] for r in o_games} == {u: r["entry"] for u, r in free_games.items()}


@pytest.mark.parametrize("G", [6, 12])
def test_loaded_positions_without_a_limit_in_force_are_untouched_by_the_limit_rules(G):
    # no limit, and a limit no uid of the run reaches set before and after the load: three HIP engines and the oracle, one
    # run, through the loaded games' ends and the ordinary games that follow them
    boards, plies = cohort_positions(G, G // 2)
    oe, ga = pair(G)
    gb, gc = pair(G)[1], pair(G)[1]
    for e in (oe, ga):
        e.set_positions(boards, plies)
    gb.set_game_limit(1 << 31)
    gb.set_positions(boards, plies)
    gc.set_positions(boards, plies)
    gc.set_game_limit(1 << 31)
    assert gsnap(ga) == gsnap(gb) == gsnap(gc)
    o_games, g_lines, _ = drive(ga, oe, twins=[gb, gc], iterations=1500, check_every=47)
    st = ga.stats()
    assert st["games"] + st["dropped"] > G and len(g_lines) > 0
    assert_lines_are_the_oracles_complete_games(g_lines, o_games)


def test_arena_engine_hands_out_the_cohorts_partial_records_and_no_other():
    # FLAG_ARENA: the games from loaded positions ARE handed out (a match from openings), marked by slot and uid
    G, N = 6, 5
    boards, plies = cohort_positions(G, N, fen=orc.START_FEN_PLAIN)
    free = pair(G, flags=orc.FLAG_ARENA, fen=orc.START_FEN_PLAIN, weight=0.0)[0]
    free.set_positions(boards, plies)
    ended = {}
    for it in range(6000):                      # precondition on the oracle without a limit: the stray would end first
        free.select()
        free.backup(*synthetic_evals(free.leaf_boards()))
        ended.update({g: it for g in range(G) if g not in ended and free.game_state(g).uid != g})
        if len(ended) == G:
            break
    assert ended[5] < max(ended[g] for g in range(N))
    oe, ge = pair(G, flags=orc.FLAG_ARENA, fen=orc.START_FEN_PLAIN, weight=0.0)
    for e in (oe, ge):
        e.set_game_limit(N)
        e.set_positions(boards, plies)
    assert phases(ge) == [0] * N + [3]
    o_games, g_lines, live = drive(ge, oe)
    assert live == set(range(N))
    st = ge.stats()
    assert st["games"] + st["dropped"] == N == len(g_lines)
    got = {e["uid"]: e for e in map(json.loads, g_lines)}
    assert sorted(got) == list(range(N))
    for rec in o_games:
        e = got[rec["uid"]]
        assert e["slot"] == rec["slot"] and {k: e[k] for k in ("boards", "dists", "moves", "result")} == rec["entry"]
        assert e["boards"][0] == cells_of(boards[rec["uid"]])
    # raised: the sixth game is the one the slot was loaded with
    for e in (oe, ge):
        e.set_game_limit(G)
    o_games, g_lines, live = drive(ge, oe)
    assert live == {5} and len(g_lines) == 1
    last = json.loads(g_lines[0])
    assert last["uid"] == 5 and last["boards"][0] == cells_of(boards[5]) and last["moves"] == o_games[0]["entry"]["moves"]


@pytest.mark.parametrize("mode", ["playout_cap", "random_symmetry", "eval_cache"])
def test_resumed_slots_in_the_modes_that_write_per_game_words_at_a_games_start(mode):
    """The playout cap (the ply's kind word), the random symmetry (the game's key word) and the evaluation cache (arena 0's
    table) each write something where a game starts.  A slot that was idled with its loaded game and resumed — before anything
    ran, or after the cohort had ended — must play the game the slot of an engine plays that had the high limit all along:
    equal word for word while both run, and equal slot for slot once all games are over."""
    G, N = 12, 6
    boards, plies = cohort_positions(G, N)
    flags = orc.FLAG_EVAL_CACHE if mode == "eval_cache" else 0
    visits = 32 if mode == "eval_cache" else 8        # (the synthetic evaluator's searches meet no transposition below some 30 visits)

    def switch_on(e):
        if mode == "playout_cap":
            e.set_playout_cap(3, 32768)
        elif mode == "random_symmetry":
            e.set_random_symmetry(True)

    oe, ga = pair(G, flags=flags, visits=visits)
    gb, gc, gd = (pair(G, flags=flags, visits=visits)[1] for _ in range(3))
    # a: idled, the mode switched on while idle, resumed before any step; b: the high limit from the start
    ga.set_game_limit(N)
    ga.set_positions(boards, plies)
    switch_on(ga)
    ga.set_game_limit(G)
    gb.set_game_limit(G)
    switch_on(gb)
    gb.set_positions(boards, plies)
    # c: the mode on first, loaded, limited, resumed
    switch_on(gc)
    gc.set_positions(boards, plies)
    gc.set_game_limit(N)
    gc.set_game_limit(G)
    lock = oe if mode == "eval_cache" else None       # (the oracle has the cache; the other two modes are the engine's own)
    if lock is not None:
        oe.set_positions(boards, plies)
        oe.set_game_limit(G)
    _, _, live = drive(ga, lock, twins=[gb, gc])
    assert live == set(range(G))
    final = gsnap(ga)
    st = final[1]
    assert st["games"] + st["dropped"] == G
    if mode == "eval_cache":
        assert st["cache_hits"] > 0
    # d: the cohort first, the rest resumed after it had ended — other iterations, the same games: every slot ends where
    # a's did, and the counters (sums over the games) agree
    switch_on(gd)
    gd.set_game_limit(N)
    gd.set_positions(boards, plies)
    _, _, live = drive(gd)
    assert live == set(range(N)) and gd.stats()["games"] + gd.stats()["dropped"] == N
    gd.set_game_limit(G)
    assert phases(gd) == [3] * N + [0] * (G - N)
    _, _, live = drive(gd)
    assert live == set(range(N, G))
    assert gsnap(gd) == final


def test_device_resident_loop_equals_host_stepping_under_a_limit_with_loaded_positions():
    # azh_engine_run (the fused tree kernel, the moves played inside the tower launch) against select / eval / backup and
    # against the oracle, f32 tower: the idle slots stay idle in the loop the CLIs run
    G, N = 12, 7
    boards, plies = cohort_positions(G, N)
    conv, bn = model.random_init(1, 128, seed=5)
    net = link.Net(conv, bn)
    oe, ga = pair(G, visits=6)
    gb = pair(G, visits=6)[1]
    for e in (oe, ga, gb):
        e.set_positions(boards, plies)
        e.set_game_limit(N)
    for chunk in range(60):
        ga.run(net, 25, link.DTYPE_F32)
        for _ in range(25):
            gb.select()
            gb.eval(net, link.DTYPE_F32)
            gb.backup()
        _oracle_follow(oe, net, oe.cfg.blockers, 25)
        ga.sync()
        compare_all(oe, ga, range(G))
        # (states and trees: the marks the two launch structures leave in the raw edge records are each one's own)
        assert [x[:2] for x in gsnap(ga, stats=False)] == [x[:2] for x in gsnap(gb, stats=False)], chunk
        assert {k: ga.stats()[k] for k in oe.stats()} == {k: gb.stats()[k] for k in oe.stats()}, chunk
        assert phases(ga)[N:] == [3] * (G - N)
        for g in range(N, G):
            assert_loaded_and_idle(ga, g, boards, plies)
        if phases(ga) == [3] * G:
            break
    assert phases(ga) == [3] * G
    so, sg = oe.stats(), ga.stats()
    for k in so:
        assert so[k] == sg[k], (k, so[k], sg[k])
    assert sg["games"] + sg["dropped"] == N and ga.drain_json() == []
    popped = [r["uid"] for r in oe.pop_games(partial=True)]
    assert len(popped) == sg["games"] and set(popped) <= set(range(N))
    for e in (oe, ga):
        e.set_game_limit(G)
    assert phases(ga) == [3] * N + [0] * (G - N)
    ga.run(net, 25, link.DTYPE_F32)
    _oracle_follow(oe, net, oe.cfg.blockers, 25)
    ga.sync()
    compare_all(oe, ga, range(G))
    net.close()


@pytest.mark.parametrize("loaded", [True, False])
def test_a_fresh_root_left_by_a_host_played_move_is_a_game_that_has_begun(loaded):
    """azh_engine_play_moves on a root nobody has searched leaves AZH_PLAY_FRESH: phase 0, one node, no visits, the record
    start moved to the new ply — the words of a loaded game that has not begun, but a move of the game HAS been played.  The
    limit does not stop it: the engine equals a twin that was never given the limit."""
    G, N = 6, 3
    boards, plies = cohort_positions(G, N, late_empty=10)
    a, twin = pair(G)[1], pair(G)[1]

    def goes_on(board, mv):     # the position after `mv` is not a finished one
        p = orc.pos_from_fen(orc.START_FEN_SELFPLAY)
        p.pieces[0], p.pieces[1], p.turn = int(board[0]) & ((1 << 63) - 1), int(board[1]), int(board[0]) >> 63
        orc.lib().orc_makemove(p, mv & 0xFF, mv >> 8)
        return orc.result(p) == 0

    for e in (a, twin):
        if loaded:
            e.set_positions(boards, plies)
        moves = np.array([next(int(m) for m in r.moves if goes_on(e.tree(g)[0][0], int(m))) for g, r in enumerate(e.root_report())],
                         dtype=np.uint16)
        assert (e.play_moves(moves) == link.PLAY_FRESH).all()
    for g in range(G):
        s = a.game_state(g)
        assert (s.phase, s.n_nodes, s.root_visits, s.ply, s.uid) == (0, 1, 0, (plies[g] if loaded else 0) + 1, g)
    a.set_game_limit(N)
    assert 3 not in phases(a) and gsnap(a) == gsnap(twin)
    # both play on alike until the first slot of `a` has ended its game and gone idle
    for it in range(3000):
        gstep(a)
        gstep(twin)
        if 3 in phases(a):
            break
        if it % 17 == 0:
            assert gsnap(a) == gsnap(twin), it
    idle = [g for g in range(G) if a.game_state(g).phase == 3]
    assert idle and all(a.game_state(g).uid == g + G for g in idle)
    rest = [g for g in range(G) if g not in idle]
    assert [gsnap(a, stats=False)[g] for g in rest] == [gsnap(twin, stats=False)[g] for g in rest]
