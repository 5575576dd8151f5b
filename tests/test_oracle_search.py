"""Oracle search engine: invariants the reference's algorithm implies (the oracle is the
checker for the HIP engine, so it is itself checked against the reference's semantics)."""
import numpy as np
import pytest

from oracle import oracle_lib as orc
from tests.helpers import replay_game_entry, synthetic_evals
from tests.limit_fixtures import LIMIT_CASES, LIMIT_PLIES, cells_of, free_run, limit_engine, step


def run(e, iters, evaluator):
    games = []
    for _ in range(iters):
        e.select()
        logits, values = evaluator(e.leaf_boards())
        e.backup(logits, values)
        games += e.pop_games()
    return games


def null_eval(lb):
    return np.zeros((len(lb), 833), np.float32), np.zeros(len(lb), np.float32)


def test_philox_known_answers_and_detmath_accuracy():
    out = np.zeros(4, np.uint32)
    orc.lib().orc_probe_philox(0, 0, 0, 0, 0, out.ctypes.data)
    assert [hex(v) for v in out] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    orc.lib().orc_probe_philox(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, out.ctypes.data)
    assert [hex(v) for v in out] == ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]
    xs = np.random.default_rng(0).uniform(-80, 80, 500).astype(np.float32)
    e = np.array([orc.lib().orc_probe_expf(float(x)) for x in xs])
    assert np.allclose(e, np.exp(xs.astype(np.float64)), rtol=3e-7)
    g = np.array([orc.lib().orc_probe_gamma(0.15, 1, i, 0, 0) for i in range(20000)])
    assert abs(g.mean() - 0.15) < 0.01 and abs(g.var() - 0.15) < 0.02  # Gamma(0.15,1)


def test_games_replay_and_root_visits_reach_threshold():
    e = orc.Engine(orc.make_config(games=12, visits=20, seed=3))
    games = run(e, 2500, synthetic_evals)
    assert len(games) >= 6
    st = e.stats()
    assert st["games"] == len(games) and st["edge_overflow"] == 0
    # NN evals per ply = steps that reached a new non-terminal node + 1 root refresh (:489-490)
    assert st["nn_evals"] <= st["steps"] + st["plies"] + 12
    for rec in games:
        entry = rec["entry"]
        assert replay_game_entry(entry, orc.START_FEN_SELFPLAY) == entry["result"] and entry["result"] in (1, 2)
        assert all(abs(sum(d.values()) - 1) < 1e-12 for d in entry["dists"])


def test_tree_invariants_during_search():
    e = orc.Engine(orc.make_config(games=4, visits=50, seed=8))
    for it in range(260):
        e.select()
        logits, values = synthetic_evals(e.leaf_boards())
        e.backup(logits, values)
        if it % 20 != 19:
            continue
        for g in range(4):
            s = e.game_state(g)
            boards, info, edges, moves = e.tree(g)
            assert s.n_nodes <= e.node_cap and s.n_nodes <= 50 + 2  # nodes <= visits + 1
            first, m = info[0, 0], info[0, 1] & 0xFFFF
            root_edges = edges[first:first + m]
            assert int(root_edges[:, 1].sum()) == s.root_visits  # all_edge_visits == sum of edge visits
            if s.phase == 1:
                pri = root_edges[:, 0].copy().view(np.float32)
                assert abs(float(pri.sum()) - 1.0) < 1e-4  # priors renormalised over legal moves (:241-245)
            # every child pointer is a valid node and each node has one parent
            kids = edges[:, 3][edges[:, 3] != 0xFFFFFFFF]
            assert len(set(kids.tolist())) == len(kids) == s.n_nodes - 1
            # W / n in [0, 1]: scores are probabilities of winning (:447)
            n = edges[:, 1].astype(np.float64)
            w = edges[:, 2].copy().view(np.float32).astype(np.float64)
            assert ((w >= -1e-6) & (w <= n + 1e-4)).all()


def test_dirichlet_noise_only_at_root_and_null_net_uniform_priors():
    e = orc.Engine(orc.make_config(games=2, visits=30, seed=1, weight=0.0))
    e.select()
    e.backup(*null_eval(e.leaf_boards()))
    boards, info, edges, moves = e.tree(0)
    m = info[0, 1] & 0xFFFF
    pri = edges[:m, 0].copy().view(np.float32)
    assert np.allclose(pri, 1.0 / m, rtol=1e-6)  # zero logits -> uniform over legal moves
    e2 = orc.Engine(orc.make_config(games=2, visits=30, seed=1, weight=0.25))
    e2.select()
    e2.backup(*null_eval(e2.leaf_boards()))
    pri2 = e2.tree(0)[2][:m, 0].copy().view(np.float32)
    assert abs(pri2.sum() - 1) < 1e-5 and pri2.std() > 1e-3 and (pri2 >= 0.75 / m - 1e-6).all()


def test_plies_cap_drops_games():
    e = orc.Engine(orc.make_config(games=6, visits=4, seed=2, max_plies=10))
    games = run(e, 400, synthetic_evals)
    st = e.stats()
    assert st["dropped"] > 0 and all(len(r["entry"]["moves"]) <= 10 for r in games)


def test_one_random_move_variant():
    # ONE_RANDOM_MOVE (cpp/self_play_client.cpp:515-552): random_ply uniform on 0..119; after it
    # the move played is the most visited one; at it any legal move (replay validates legality)
    cfg = orc.make_config(games=48, visits=8, seed=3, max_plies=150, flags=orc.FLAG_ONE_RANDOM_MOVE)
    e = orc.Engine(cfg)
    games = run(e, 2600, null_eval)
    assert len(games) >= 20
    rps = [g["entry"]["random_ply"] for g in games]
    assert all(0 <= r < 120 for r in rps) and len(set(rps)) > 10
    after = 0
    for g in games:
        en = g["entry"]
        assert replay_game_entry(en, orc.START_FEN_SELFPLAY) == en["result"]
        for ply in range(en["random_ply"] + 1, len(en["moves"])):
            d = en["dists"][ply]
            assert d[en["moves"][ply]] == max(d.values())
            after += 1
    assert after > 50
    # a different game uid draws a different ply; same seed + uid reproduces it
    e2 = orc.Engine(cfg)
    games2 = run(e2, 2600, null_eval)
    assert [g["entry"] for g in games2] == [g["entry"] for g in games]


def test_select_budget_changes_timing_not_games():
    # parked descents (select_budget) resume on an unchanged tree: per game the same search, the same record
    def play(budget, iters):
        e = orc.Engine(orc.make_config(games=8, visits=12, seed=12, max_plies=300, select_budget=budget))
        return {g["uid"]: g["entry"] for g in run(e, iters, synthetic_evals)}, e
    base, e0 = play(0, 6000)
    slow, e1 = play(2, 12000)
    common = set(base) & set(slow)
    assert len(common) >= 4
    for uid in common:
        assert base[uid] == slow[uid]
    assert e1.stats()["steps"] < 12000 * 8  # some iterations were spent parked


def test_root_noise_is_dirichlet_and_moves_follow_the_visits():
    """The two random ingredients of the C++ generator that no reference vector can pin (unseeded RNG there) are
    checked against their DEFINITIONS with third-party statistics: the gamma draws behind the root noise
    (std::gamma_distribution(0.15, 1), cpp/self_play_client.cpp:252-255) against scipy's Gamma(0.15) by a
    Kolmogorov-Smirnov test, and the move sampler (:495-506) against the visit counts by a chi-square test."""
    from scipy import stats
    g = np.array([orc.lib().orc_probe_gamma(0.15, 12345, uid, 3, uid % 50) for uid in range(20000)], dtype=np.float64)
    assert (g >= 0).all() and abs(g.mean() - 0.15) < 0.01 and abs(g.var() - 0.15) < 0.02
    # (the smallest draws underflow to 0 in f32; Gamma(0.15) puts ~1.5 % of its mass below 1e-12)
    assert stats.kstest(g[g > 1e-12], lambda x: (stats.gamma.cdf(x, 0.15) - stats.gamma.cdf(1e-12, 0.15)) /
                        (1 - stats.gamma.cdf(1e-12, 0.15))).pvalue > 1e-3
    # move ~ visits / N: many one-ply games from the same position with a pure-function evaluator and no noise give the same
    # root visit counts in every slot, so the played moves are i.i.d. samples of that one distribution
    from tests.helpers import synthetic_evals
    G = 6000
    e = orc.Engine(orc.make_config(games=G, visits=60, seed=99, weight=0.0, max_plies=400))
    tree0 = None
    while e.stats()["plies"] < G:
        e.select()
        e.backup(*synthetic_evals(e.leaf_boards()))
        if tree0 is None and e.game_state(0).phase == 2:
            b, info, edges, moves = e.tree(0)
            first, m = int(info[0, 0]), int(info[0, 1] & 0xFFFF)
            tree0 = (moves[first:first + m].copy(), edges[first:first + m, 1].astype(np.float64))
    # the first move of every slot's game is recorded in its ply-0 record: read it back through the kept subtrees' roots
    played = {}
    for gme in range(G):
        s = e.game_state(gme)
        assert s.ply == 1
        x = int(e.tree(gme)[0][0, 0]) & ((1 << 63) - 1)
        played[x] = played.get(x, 0) + 1
    mv, n = tree0
    p0 = orc.pos_from_fen(orc.START_FEN_SELFPLAY)
    expect = {}
    for m_, cnt in zip(mv, n):
        q = orc.Pos()
        q.pieces[0], q.pieces[1], q.blockers, q.turn = p0.pieces[0], p0.pieces[1], p0.blockers, p0.turn
        orc.lib().orc_makemove(q, int(m_) & 0xFF, int(m_) >> 8)
        expect[int(q.pieces[0])] = expect.get(int(q.pieces[0]), 0) + cnt / n.sum() * G
    keys = sorted(k for k, v in expect.items() if v > 0)
    assert set(played) <= set(keys) and len(keys) >= 4
    obs = np.array([played.get(k, 0) for k in keys], dtype=np.float64)
    exp = np.array([expect[k] for k in keys])
    assert stats.chisquare(obs, exp).pvalue > 1e-3


def test_evaluation_cache_changes_no_tree():
    """ORC_FLAG_EVAL_CACHE (engine.py's NNEvaluator.cache, per game): with a deterministic evaluator the cached search
    builds exactly the trees of the uncached one — every board, move, prior, visit count and score, iteration for
    iteration — while a good share of the expansions never reaches the evaluator."""
    from tests.helpers import synthetic_evals
    a = orc.Engine(orc.make_config(games=12, visits=120, seed=5))
    b = orc.Engine(orc.make_config(games=12, visits=120, seed=5, flags=orc.FLAG_EVAL_CACHE))
    asked_a = asked_b = 0
    for it in range(900):
        na, need_a = a.select()
        nb, need_b = b.select()
        asked_a += na
        asked_b += nb
        assert ((need_b == 0) | (need_a == need_b)).all()          # the cache only ever removes evaluations
        la, lb = a.leaf_boards(), b.leaf_boards()
        assert (la == lb).all()
        a.backup(*synthetic_evals(la))
        b.backup(*synthetic_evals(lb))
        if it % 60 == 0 or it == 899:
            for g in range(12):
                ta, tb = a.tree(g), b.tree(g)
                assert (ta[0] == tb[0]).all() and (ta[2] == tb[2]).all() and (ta[3] == tb[3]).all()
                assert (ta[1][:, :3] == tb[1][:, :3]).all()            # node_info[3] also keeps the value when caching
    sa, sb = a.stats(), b.stats()
    assert sa["steps"] == sb["steps"] and sa["plies"] == sb["plies"] >= 60
    assert sb["cache_hits"] > 0 and sb["nn_evals"] + sb["cache_hits"] == sa["nn_evals"] and asked_b < asked_a
    # (few with this peaked synthetic evaluator; about a quarter of the expansions with a real net: tools/leaf_duplicates.py)


def test_game_limit_plays_exactly_the_games_below_it():
    # orc_engine_set_game_limit (mirror of azh_engine_set_game_limit): uids 0 .. N - 1 and nothing else; slots idle afterwards
    from tests.helpers import synthetic_evals
    e = orc.Engine(orc.make_config(8, 4, seed=3, max_plies=60))
    e.set_game_limit(20)
    uids = set()
    for _ in range(4000):
        _, need = e.select()
        uids |= {e.game_state(g).uid for g in range(8) if e.game_state(g).phase != 3}
        lg, v = synthetic_evals(e.leaf_boards())
        e.backup(lg, v)
        st = e.stats()
        if st["games"] + st["dropped"] >= 20:
            break
    assert st["games"] + st["dropped"] == 20 and uids == set(range(20))
    assert all(e.game_state(g).phase == 3 and e.game_state(g).uid >= 20 for g in range(8))
    n, need = e.select()
    assert n == 0 and not need.any()
    lg, v = synthetic_evals(e.leaf_boards())
    e.backup(lg, v)
    assert e.stats() == st
    # raising the limit wakes the idle slots whose next game is now below it
    e.set_game_limit(23)
    awake = sorted(e.game_state(g).uid for g in range(8) if e.game_state(g).phase != 3)
    assert awake == [20, 21, 22]
    for _ in range(4000):
        e.select()
        lg, v = synthetic_evals(e.leaf_boards())
        e.backup(lg, v)
        st = e.stats()
        if st["games"] + st["dropped"] >= 23:
            break
    assert st["games"] + st["dropped"] == 23 and all(e.game_state(g).phase == 3 for g in range(8))


# ---------------------------------------------------------------- the game limit with loaded positions
# orc_engine_set_game_limit together with orc_engine_set_positions (mcts_oracle.h): a loaded slot past the limit
# that has not begun is idle whichever call came first, keeps what it was loaded with, resumes THAT game when the limit is
# raised, and adds nothing to any counter meanwhile.  tests/test_gpu_game_limit.py repeats every case in lock step with the
# HIP engine; here the rules are stated on the oracle alone.


def snapshot(e):
    """every slot's state words and tree arrays, and the counters"""
    return [(e.game_state(g).as_tuple(), [a.tobytes() for a in e.tree(g)]) for g in range(e.G)], e.stats()


def play_out(e, max_iters=6000):
    """Steps until every slot is idle.  -> (games popped, partial ones included, by uid; uids seen in a slot that was not idle;
    iteration at which each uid left its slot)"""
    games, live, ended = {}, set(), {}
    uid_of = [e.game_state(g).uid for g in range(e.G)]
    for it in range(max_iters):
        states = [e.game_state(g) for g in range(e.G)]
        live |= {s.uid for s in states if s.phase != 3}
        if all(s.phase == 3 for s in states):
            break
        step(e)
        for g in range(e.G):
            u = e.game_state(g).uid
            if u != uid_of[g]:
                ended[uid_of[g]] = it
                uid_of[g] = u
        for rec in e.pop_games(partial=True):
            assert rec["uid"] not in games
            games[rec["uid"]] = rec
    else:
        raise AssertionError("slots still playing after %d iterations" % max_iters)
    return games, live, ended


def assert_loaded_and_idle(e, g, boards, plies):
    s = e.game_state(g)
    assert (s.phase, s.uid, s.ply, s.n_nodes, s.root_visits, s.leaf_kind) == (3, g, plies[g], 1, 0, orc.LEAF_NONE), (g, s.as_tuple())
    assert (e.tree(g)[0][0] == boards[g]).all(), g


@pytest.mark.parametrize("G,N", LIMIT_CASES)
def test_game_limit_idles_loaded_slots_in_either_call_order_and_plays_the_cohort_alone(G, N):
    from tests.helpers import cohort_positions
    boards, plies = cohort_positions(G, N)
    assert plies.max() < LIMIT_PLIES and len(set(plies.tolist())) > 2
    # precondition, on the engine without a limit: a game past the limit would end before the cohort's last one does — an
    # engine that plays it hands it out and counts it while the match is still running
    free_games, free_end = free_run(G, N)
    assert min(free_end[g] for g in range(N, G)) < max(free_end[g] for g in range(N))
    a, b = limit_engine(G), limit_engine(G)
    a.set_positions(boards, plies)
    a.set_game_limit(N)
    b.set_game_limit(N)
    b.set_positions(boards, plies)
    assert snapshot(a) == snapshot(b)
    for e in (a, b):
        for g in range(G):
            if g >= N:
                assert_loaded_and_idle(e, g, boards, plies)
            else:
                s = e.game_state(g)
                assert (s.phase, s.uid, s.ply) == (0, g, plies[g]) and (e.tree(g)[0][0] == boards[g]).all()
    games_a, live_a, _ = play_out(a)
    games_b, live_b, _ = play_out(b)
    assert live_a == live_b == set(range(N))
    st = a.stats()
    assert st == b.stats() and st["games"] + st["dropped"] == N
    assert snapshot(a) == snapshot(b) and games_a == games_b
    assert set(games_a) <= set(range(N)) and len(games_a) == st["games"]
    # the cohort's games are the games those uids are without a limit, each from its loaded position on
    for u, rec in games_a.items():
        assert rec["partial"] and rec["entry"] == free_games[u]["entry"] and rec["entry"]["boards"][0] == cells_of(boards[u])
    # idle for good: nothing is selected, no counter moves, the slots past the limit still hold what they were loaded with
    assert step(a) == 0 and a.stats() == st and a.pop_games(partial=True) == []
    for g in range(N, G):
        assert_loaded_and_idle(a, g, boards, plies)


@pytest.mark.parametrize("G,N", LIMIT_CASES)
def test_game_limit_raised_before_any_step_equals_the_high_limit_from_the_start(G, N):
    from tests.helpers import cohort_positions
    boards, plies = cohort_positions(G, N)
    a, b, c = limit_engine(G), limit_engine(G), limit_engine(G)
    a.set_positions(boards, plies)
    a.set_game_limit(N)
    a.set_game_limit(G)          # idled with their loaded games, and resumed before anything ran
    b.set_game_limit(G)
    b.set_positions(boards, plies)
    c.set_game_limit(N)
    c.set_positions(boards, plies)   # (the other order of getting there)
    c.set_game_limit(G)
    assert snapshot(a) == snapshot(b) == snapshot(c)
    for g in range(G):
        s = a.game_state(g)
        assert (s.phase, s.uid, s.ply) == (0, g, plies[g]) and (a.tree(g)[0][0] == boards[g]).all()
    popped = [[], [], []]
    for it in range(6000):
        if all(a.game_state(g).phase == 3 for g in range(G)):
            break
        for e, out in zip((a, b, c), popped):
            step(e)
            out += e.pop_games(partial=True)
        if it % 9 == 0:
            assert snapshot(a) == snapshot(b) == snapshot(c), it
    assert snapshot(a) == snapshot(b) == snapshot(c) and popped[0] == popped[1] == popped[2]
    st = a.stats()
    assert st["games"] + st["dropped"] == G and len(popped[0]) == st["games"]
    free_games, _ = free_run(G, N)
    assert {r["uid"]: r["entry"] for r in popped[0]} == {u: r["entry"] for u, r in free_games.items()}


@pytest.mark.parametrize("G,N", LIMIT_CASES)
def test_game_limit_raised_after_the_cohort_resumes_loaded_games_and_starts_fresh_ones(G, N):
    from tests.helpers import cohort_positions
    boards, plies = cohort_positions(G, N)
    e = limit_engine(G)
    e.set_game_limit(N)
    e.set_positions(boards, plies)
    play_out(e)
    first = e.stats()
    assert first["games"] + first["dropped"] == N
    # raised past the slot count: the slots idled with a loaded game resume it; slots 0 and 1, whose loaded games are over,
    # start their next game (uids G, G + 1) at the start position; every other slot stays idle
    e.set_game_limit(G + 2)
    start = orc.pos_from_fen(orc.START_FEN_SELFPLAY)
    for g in range(G):
        s = e.game_state(g)
        if g >= N:
            assert (s.phase, s.uid, s.ply, s.n_nodes, s.root_visits) == (0, g, plies[g], 1, 0), (g, s.as_tuple())
            assert (e.tree(g)[0][0] == boards[g]).all()
        elif g < 2:
            assert (s.phase, s.uid, s.ply, s.n_nodes, s.root_visits) == (0, G + g, 0, 1, 0), (g, s.as_tuple())
            assert [int(v) for v in e.tree(g)[0][0]] == [int(start.pieces[0]) | (start.turn << 63), int(start.pieces[1])]
        else:
            assert (s.phase, s.uid) == (3, G + g)
    assert e.stats() == first
    games, live, _ = play_out(e)
    assert live == set(range(N, G)) | {G, G + 1}
    st = e.stats()
    assert st["games"] + st["dropped"] == G + 2 and len(games) == st["games"] - first["games"]
    free_games, _ = free_run(G, N)
    for u, rec in games.items():
        if u < G:
            # the game it was loaded with: the record starts at the loaded ply, and is the game that uid is without a limit
            assert rec["partial"] and rec["entry"]["boards"][0] == cells_of(boards[u]) and rec["entry"] == free_games[u]["entry"]
        else:
            assert not rec["partial"] and replay_game_entry(rec["entry"], orc.START_FEN_SELFPLAY) == rec["entry"]["result"]
    assert {u for u in free_games if u >= N} == {u for u in games if u < G}


@pytest.mark.parametrize("G,N", LIMIT_CASES)
def test_game_limit_never_stops_a_loaded_game_whose_root_has_been_evaluated(G, N):
    from tests.helpers import cohort_positions
    boards, plies = cohort_positions(G, N)
    e, twin = limit_engine(G), limit_engine(G)
    for x in (e, twin):
        x.set_positions(boards, plies)
        step(x)
    before = snapshot(e)
    e.set_game_limit(N)
    assert snapshot(e) == before == snapshot(twin)          # begun: the root evaluation is done, nothing is idled
    assert all(e.game_state(g).phase != 3 for g in range(G))
    games, live, _ = play_out(e)
    assert live == set(range(G))
    st = e.stats()
    assert st["games"] + st["dropped"] == G and len(games) == st["games"]
    free_games, _ = free_run(G, N)
    assert {u: r["entry"] for u, r in games.items()} == {u: r["entry"] for u, r in free_games.items()}
    # and one whose root evaluation is in flight (selected, not yet backed up) is not idled either
    f = limit_engine(G)
    f.set_positions(boards, plies)
    f.select()
    f.set_game_limit(N)
    assert all(f.game_state(g).phase != 3 for g in range(G))


@pytest.mark.parametrize("G", [6, 12])
def test_loaded_positions_without_a_limit_in_force_are_untouched_by_the_limit_rules(G):
    # no limit, a limit no uid of the run reaches, and a limit of exactly G at load time: three engines, one run, through
    # the loaded games' ends and the ordinary games that follow them
    from tests.helpers import cohort_positions
    boards, plies = cohort_positions(G, G // 2)
    a, b, c = limit_engine(G), limit_engine(G), limit_engine(G)
    a.set_positions(boards, plies)
    b.set_game_limit(1 << 31)
    b.set_positions(boards, plies)
    c.set_positions(boards, plies)
    c.set_game_limit(1 << 31)
    assert snapshot(a) == snapshot(b) == snapshot(c)
    popped = [[], [], []]
    for it in range(1500):
        for e, out in zip((a, b, c), popped):
            step(e)
            out += e.pop_games(partial=True)
        if it % 11 == 0:
            assert snapshot(a) == snapshot(b) == snapshot(c), it
    assert snapshot(a) == snapshot(b) == snapshot(c) and popped[0] == popped[1] == popped[2]
    st = a.stats()
    assert st["games"] + st["dropped"] > G and any(not r["partial"] for r in popped[0])
    # (a limit of exactly G: the first G games are the same, then the slots idle)
    d = limit_engine(G)
    d.set_game_limit(G)
    d.set_positions(boards, plies)
    assert snapshot(d)[0] == snapshot(limit_engine_loaded(G, boards, plies))[0]
    games, live, _ = play_out(d)
    assert live == set(range(G)) and {u: r["entry"] for u, r in games.items()} == \
        {r["uid"]: r["entry"] for r in popped[0] if r["uid"] < G}


def limit_engine_loaded(G, boards, plies):
    e = limit_engine(G)
    e.set_positions(boards, plies)
    return e
