"""The recorded search value and resignation on the MI355X (azh_engine_set_resign): recording changes no game, every
recorded value is W_b / n_b of the root report, games resign exactly where the numpy restatement of the rule
(tests/resign_reference.py) says, play-through games are the ones link.resign_playthrough names, the playout cap's FAST
plies do not count, the device loop equals host stepping, the K-leaf search, values that are not finite, off is the parent,
and the refusals."""
import functools
import json
import math
import re

import numpy as np
import pytest

from ataxxzero_amd import link
from tests import engine_harness as eh
from tests import helpers
from tests import resign_reference as ref
from tests.engine_harness import SEED

pytestmark = pytest.mark.gpu

KIND_CAP, KIND_VALUES, KIND_RESIGNED = link.REC_KIND_PLAYOUT_CAP, link.REC_KIND_VALUES, link.REC_KIND_RESIGNED


def _strip_values(line):
    return re.sub(rb',"values":\[[^\]]*\]', b"", line)


def _collect(e, recs, lines):
    e.fetch()
    recs += eh.records(e.staged_records())
    lines += e.drain_json()


# ------------------------------------------------------------------ 1. recording changes no game

@functools.lru_cache(maxsize=None)
def _recorded_run():
    """Run 1: A records values (every game plays through), B has the mode off; one game slot, the step-wise API with the
    synthetic evaluator, three complete games.  -> (A's lines, B's lines, {(uid, ply): (q, visited?, mover)} from B's root
    report in the iteration before each move, ties between most-visited edges seen, A's resign stats)."""
    visits = 16
    a = eh.root_engine(1, visits, weight=0.0, resign=(0.3, 2, 65536))
    b = eh.root_engine(1, visits, weight=0.0)
    lines_a, lines_b, expect, ties = [], [], {}, 0
    for it in range(8000):
        sb = b.game_state(0)
        if sb.phase == 2:                      # the move is due: the next select plays it from this root
            rep = b.root_report(0, 1)[0]
            q, visited = ref.ply_value(rep.visits, rep.scores)
            ties += int((rep.visits == rep.visits.max()).sum() > 1)
            mover = 1 + (int(b.tree(0)[0][0][0]) >> 63)
            assert mover == eh.mover(sb.ply)
            expect[(sb.uid, sb.ply)] = (q, visited, mover)
        eh.step(a)
        eh.step(b)
        eh.same(eh.dump(a), eh.dump(b))
        lines_a += a.drain_json()
        lines_b += b.drain_json()
        if len(lines_b) >= 3:
            break
    stats = a.resign_stats()
    off_stats = b.resign_stats()
    a.close(), b.close()
    return lines_a, lines_b, expect, ties, stats, off_stats


def test_recording_changes_no_game_and_the_value_is_the_root_reports():
    lines_a, lines_b, expect, ties, stats, off_stats = _recorded_run()
    assert len(lines_a) == len(lines_b) >= 3
    assert ties > 0                            # the most visited edge was not unique at least once: the lowest index
    checked = 0
    for uid, (la, lb) in enumerate(zip(lines_a, lines_b)):
        assert b"values" not in lb and b"resigned" not in la and _strip_values(la) == lb
        ea = json.loads(la)
        assert list(ea.keys()) == ["boards", "dists", "moves", "result", "values"]
        assert len(ea["values"]) == len(ea["moves"])
        for ply, v in enumerate(ea["values"]):
            q, visited, _ = expect[(uid, ply)]
            assert visited and v == 2 * float(np.float32(q)) - 1, (uid, ply)
            checked += 1
    assert checked > 30
    assert stats["resigned"] == 0 and stats["playthrough"] == len(lines_a)
    assert off_stats == {"resigned": 0, "playthrough": 0, "playthrough_fired": 0, "playthrough_false": 0}


# ------------------------------------------------------------------ 2. resigning

def test_games_resign_where_the_rule_says_and_the_slot_restarts():
    """The threshold is the 0.05 quantile of the values run 1 recorded on its counted plies (every ply: no playout cap), as
    q = (v + 1) / 2: one ply in twenty is bad, so two bad plies of a side in a row are a losing side's and not every game
    has them — of the 33 games some resign and some reach their real end (the 0.2 quantile ends all 33 by ply 13).  Each
    slot's first game (uid = slot) is followed in lock step with a mode-off engine up to the ply the reference rule names
    on B's own root reports."""
    lines_a = _recorded_run()[0]
    qs = np.array([(v + 1) / 2 for l in lines_a for v in json.loads(l)["values"]], dtype=np.float32)
    t = float(np.quantile(qs, 0.05))
    G, visits = 33, 16
    a = eh.root_engine(G, visits, weight=0.0, resign=(t, 2, 0))
    b = eh.root_engine(G, visits, weight=0.0)
    seq = [[] for _ in range(G)]               # B's plies as the rule takes them
    live = set(range(G))                       # slots whose first game A and B still play together
    resigned_at = {}
    recs_a, recs_b, lines_a2, lines_b2 = [], [], [], []
    for it in range(4000):
        sb = [b.game_state(g) for g in range(G)]
        if all(s.uid != g for g, s in enumerate(sb)) and not live:
            break
        reports = b.root_report()
        due = {}
        for g in sorted(live):
            if sb[g].phase == 2 and sb[g].uid == g:
                q, visited = ref.ply_value(reports[g].visits, reports[g].scores)
                seq[g].append((eh.mover(sb[g].ply), ref.q_bits(q), visited))
                assert len(seq[g]) == sb[g].ply + 1
                due[g] = ref.replay(seq[g], t, 2)[-1]
        eh.step(a)
        eh.step(b)
        for g in sorted(live):
            sa, sb2 = a.game_state(g), b.game_state(g)
            if due.get(g):
                # the rule fired at the ply just played: A's game ended there, the slot restarted, B simply goes on
                assert (sa.uid, sa.ply, sa.root_visits, sa.n_nodes, sa.phase) == (g + G, 0, 0, 1, 0), (g, sa.as_tuple())
                assert sb2.uid == g + G or (sb2.uid == g and sb2.ply == len(seq[g]))
                resigned_at[g] = len(seq[g]) - 1
                live.discard(g)
            elif sb2.uid != g:
                assert sa.uid == sb2.uid           # a real end, in both
                live.discard(g)
        eh.same(eh.dump(a, sorted(live)), eh.dump(b, sorted(live)))
        if it % 16 == 0:
            _collect(a, recs_a, lines_a2)
            _collect(b, recs_b, lines_b2)
    _collect(a, recs_a, lines_a2)
    _collect(b, recs_b, lines_b2)
    first_a = {uid: (result, kind, rows) for _, uid, result, kind, rows in recs_a if uid < G}
    first_b = {uid: (result, kind, rows) for _, uid, result, kind, rows in recs_b if uid < G}
    assert set(first_b) == set(range(G)) and not live
    real = 0
    for g in range(G):
        fire = ref.first_fire(seq[g], t, 2)
        rb, kb, rows_b = first_b[g]
        assert kb == 0 and len(rows_b) >= len(seq[g]) and (fire is not None or len(rows_b) == len(seq[g]))
        ra, ka, rows_a = first_a[g]
        strip = lambda rows: [(m, c, bd) for m, _, c, bd in rows]
        if fire is None:
            assert g not in resigned_at and ka == KIND_VALUES and ra == rb and strip(rows_a) == strip(rows_b)
            real += 1
        else:
            p, mover = fire
            assert resigned_at[g] == p and ka == KIND_VALUES | KIND_RESIGNED
            assert len(rows_a) == p + 1 and ra == 3 - mover          # no longer, no shorter than the rule says
            assert strip(rows_a) == strip(rows_b[:p + 1])            # board, visit distribution, the sampled move
        assert [w5 for _, w5, _, _ in rows_a] == [bits for _, bits, _ in seq[g][:len(rows_a)]]
    assert len(resigned_at) >= 1 and real >= 1, (len(resigned_at), real, t)
    got = [e for e in map(json.loads, lines_a2) if "resigned" in e]
    assert len(got) == a.resign_stats()["resigned"] >= len(resigned_at)
    for e in got:
        assert list(e.keys()) == ["boards", "dists", "moves", "resigned", "result", "values"]
        assert e["resigned"] == 3 - e["result"] == eh.mover(len(e["moves"]) - 1)
    assert a.stats()["games"] == len(recs_a)
    a.close(), b.close()


# ------------------------------------------------------------------ 3. shares, 4. the playout cap

@functools.lru_cache(maxsize=None)
def _loop_threshold():
    """The threshold of the device-loop tests: the 0.3 quantile of the values a 33-game engine with the tests' random net
    records in 300 iterations with resignation off (q_below = 0) — low enough that games are played for a while, high enough
    that, with two consecutive plies of a side needed, games do resign."""
    net = eh.net()
    e = eh.root_engine(33, 16, weight=0.25, resign=(0.0, 1, 0))
    recs, lines = [], []
    e.run(net, 300, link.DTYPE_BF16)
    _collect(e, recs, lines)
    assert e.resign_stats()["resigned"] == 0 and len(recs) >= 33       # q_below = 0 records values and never resigns
    qs = np.array([ref.q_of_bits(w5) for _, _, _, _, rows in recs for _, w5, _, _ in rows], dtype=np.float32)
    e.close()
    return float(np.quantile(qs, 0.3))


@pytest.mark.parametrize("games", [5, 33, 130])
def test_play_through_games_are_the_ones_the_draw_names(games):
    t, k, share = _loop_threshold(), 2, 16384
    net = eh.net()
    e = eh.root_engine(games, 16, weight=0.25, resign=(t, k, share))
    recs, lines = [], []
    for _ in range(40):
        e.run(net, 100, link.DTYPE_BF16)
        _collect(e, recs, lines)
        if {r[0] for r in recs} == set(range(games)):
            break
    assert {r[0] for r in recs} == set(range(games))       # every slot has finished a game
    assert len(lines) == len(recs) and all(r[1] % games == r[0] for r in recs)
    stats = eh.check_resign_records(recs, t, k, share)
    assert e.resign_stats() == stats
    assert e.stats()["games"] == len(recs)
    if games >= 33:
        assert stats["resigned"] > 0 and stats["playthrough"] > 0, stats
    for line in lines:
        entry = json.loads(line)
        assert ("resigned" in entry) == (b'"resigned"' in line) and len(entry["values"]) == len(entry["moves"])
    assert sum("resigned" in json.loads(l) for l in lines) == stats["resigned"]
    e.close()


def test_fast_plies_neither_advance_nor_reset_a_counter():
    G, visits, fast, frac, t, k = 33, 16, 4, 16384, _loop_threshold(), 2
    net = eh.net()
    e = eh.root_engine(G, visits, weight=0.25, cap=(fast, frac), resign=(t, k, 0))
    recs, lines = [], []
    for _ in range(40):
        e.run(net, 100, link.DTYPE_BF16)
        _collect(e, recs, lines)
        if {r[0] for r in recs} == set(range(G)):
            break
    assert {r[0] for r in recs} == set(range(G))
    differs = fasts = fulls = 0
    for slot, uid, result, kind, rows in recs:
        assert kind & ~KIND_RESIGNED == KIND_CAP | KIND_VALUES
        for ply, (_, w5, _, _) in enumerate(rows):
            full = link.playout_cap_kind(SEED, uid, ply, frac)
            assert w5 >> 31 == full, (uid, ply)                     # word 5 carries the sign bit and the value
            assert 0.0 <= float(ref.q_of_bits(w5)) <= 1.0
            fulls += full
            fasts += 1 - full
        every = [(m, bits, True) for m, bits, _ in eh.resign_sequence(rows, kind)]
        differs += int(ref.first_fire(every, t, k) != ref.first_fire(eh.resign_sequence(rows, kind), t, k))
    stats = eh.check_resign_records(recs, t, k, 0)
    assert e.resign_stats() == stats and stats["resigned"] > 0
    assert fasts > fulls > 0 and differs > 0       # the rule over all plies would have ended games elsewhere
    for line in lines:
        entry = json.loads(line)
        assert list(entry.keys()) == ["boards", "dists", "full", "moves"] + ["resigned"] * ("resigned" in entry) + \
            ["result", "values"]
    e.close()


# ------------------------------------------------------------------ 5. device loop = host stepping, 6. K leaves

@pytest.mark.parametrize("K", [1, 4])
def test_device_loop_equals_host_stepping_with_the_mode_on(K):
    net = eh.net()
    n, G, t, k, share = 200, 33 if K == 1 else 9, _loop_threshold(), 2, 16384
    a = eh.root_engine(G, 16, weight=0.25, resign=(t, k, share), K=K)
    b = eh.root_engine(G, 16, weight=0.25, resign=(t, k, share), K=K)
    a.run(net, n, link.DTYPE_BF16)
    a.sync()
    for _ in range(n):
        b.select()
        b.eval(net, link.DTYPE_BF16)
        b.backup()
    eh.same(eh.dump(a), eh.dump(b))
    assert a.stats() == b.stats() and a.stats()["plies"] > 5 * G
    assert a.resign_stats() == b.resign_stats()
    recs, la, lb = [], [], b.drain_json()
    _collect(a, recs, la)
    assert sorted(la) == sorted(lb) and len(la) > 0 and all(b'"values":[' in l for l in la)
    assert eh.check_resign_records(recs, t, k, share) == a.resign_stats()      # records obey the rule (K leaves per game too)
    assert a.resign_stats()["resigned"] > 0
    a.close(), b.close()


# ------------------------------------------------------------------ 7. values that are not finite

def _evals_nan(lb):
    logits, values = helpers.synthetic_evals_distinct(lb)
    return logits, np.full_like(values, np.nan)


def _evals_some_infinite(lb):
    """a third of the boards evaluate to NaN, +inf or -inf"""
    logits, values = helpers.synthetic_evals_distinct(lb)
    pick = (np.asarray(lb, dtype=np.uint64).reshape(-1, 2).sum(axis=1) % np.uint64(9)).astype(np.int64)
    values = values.copy()
    values[pick == 0] = np.nan
    values[pick == 1] = np.inf
    values[pick == 2] = -np.inf
    return logits, values


@pytest.mark.parametrize("evals", [_evals_nan, _evals_some_infinite])
def test_values_that_are_not_finite(evals):
    """Every evaluation NaN (only finished positions in the tree still give a finite value), or a third of them NaN, +inf or
    -inf: a ply's q is finite, NaN or infinite.  The records obey the reference rule with its plain IEEE < — NaN and +inf
    are never below, and -inf is recorded and judged without its sign, so no game resigns at such a ply — a q that is not
    finite is written as 0, and the loop goes on."""
    G, t = 8, 0.4
    e = eh.root_engine(G, 12, weight=0.0, resign=(t, 1, 0))
    recs, lines = [], []
    for it in range(6000):
        eh.step(e, evals)
        if it % 100 == 99:
            _collect(e, recs, lines)
            if len(recs) >= G:
                break
    assert len(recs) >= G and e.stats()["plies"] > 5 * G and len(lines) == len(recs)
    assert eh.check_resign_records(recs, t, 1, 0) == e.resign_stats()
    odd, want = 0, []
    for _, _, _, kind, rows in recs:
        qs = [float(ref.q_of_bits(w5)) for _, w5, _, _ in rows]
        assert not (kind & KIND_RESIGNED) or qs[-1] < t           # never at a NaN or an infinity
        odd += sum(not math.isfinite(q) for q in qs)
        want.append([2 * q - 1 if math.isfinite(q) else 0.0 for q in qs])
    assert odd > 0
    assert sorted(json.loads(l)["values"] for l in lines) == sorted(want)
    assert not any(b"null" in l or b"NaN" in l or b"nan" in l for l in lines)
    e.close()


# ------------------------------------------------------------------ 8. off is the parent, 9. refusals

def test_switched_off_is_the_engine_without_the_mode():
    net = eh.net(seed=5)
    n, G = 400, 5
    ref_e = eh.root_engine(G, 12, weight=0.25)
    off = eh.root_engine(G, 12, weight=0.25, resign=(0.47, 2, 16384))
    off.set_resign(0.9, 0, 123)
    for e in (ref_e, off):
        e.run(net, n, link.DTYPE_F32)
        e.sync()
    eh.same(eh.dump(ref_e), eh.dump(off))
    want = ref_e.drain_json()
    assert len(want) >= G and not any(b"values" in l or b"resigned" in l for l in want)
    recs, got = [], []
    _collect(off, recs, got)
    assert got == want and all(kind == 0 for _, _, _, kind, _ in recs)        # byte for byte, no "values" key
    assert ref_e.stats() == off.stats()
    assert off.resign_stats() == {"resigned": 0, "playthrough": 0, "playthrough_fired": 0, "playthrough_false": 0}
    ref_e.close(), off.close()


def test_refusals_leave_the_engine_usable():
    e = eh.root_engine(4, 24, weight=0.0)
    for bad in [(1.0, 2, 0), (-0.1, 2, 0), (float("nan"), 2, 0), (1.5, 2, 0), (0.3, 256, 0), (0.3, -1, 0), (0.3, 2, 65537),
                (0.3, 2, -1)]:
        with pytest.raises(link.AzhError):
            e.set_resign(*bad)
        eh.step(e)
    e.set_resign(0.3, 255, 65536)
    e.set_resign(0.0, 1, 0)
    e.select()
    with pytest.raises(link.AzhError):
        e.set_resign(0.3, 2, 0)               # a selected batch awaits its backup
    with pytest.raises(link.AzhError):
        e.set_resign(0.3, 0, 0)
    need, lb = e.leaves()
    e.set_evals(*helpers.synthetic_evals_distinct(lb))
    e.backup()
    e.set_resign(0.3, 2, 0)
    for _ in range(60):
        eh.step(e)
    assert e.stats()["plies"] > 0
    e.set_resign(0.0, 0, 0)
    e.close()
    for flags in (link.FLAG_TWO_NETS, link.FLAG_ONE_RANDOM_MOVE):
        r = eh.root_engine(4, 24, weight=0.0, flags=flags)
        with pytest.raises(link.AzhError):
            r.set_resign(0.3, 2, 0)
        r.set_resign(0.0, 0, 0)               # switching off is no request for the mode
        net = eh.net()
        if flags == link.FLAG_TWO_NETS:
            r.run_arena(net, net, 20, link.DTYPE_F32)
        else:
            r.run(net, 20, link.DTYPE_F32)
        r.sync()
        assert r.stats()["steps"] > 0
        assert r.resign_stats()["resigned"] == 0
        r.close()
