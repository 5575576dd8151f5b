"""Playout cap randomization on the MI355X (azh_engine_set_playout_cap): per-ply thresholds in lock step with a host-driven
uncapped engine, records that say which plies were searched in full, root noise on FULL plies only, the leaf-parallel
batch size, the device loop against host stepping, the degenerate settings and the refusals."""
import json
import re

import numpy as np
import pytest

from ataxxzero_amd import link
from tests import engine_harness as eh
from tests import helpers
from tests.engine_harness import SEED

pytestmark = pytest.mark.gpu


def _strip_full(line):
    return re.sub(rb',"full":\[[01,]*\]', b"", line)


def test_lock_step_with_a_host_driven_uncapped_engine():
    """A (cap on) against B (cap off), whose threshold the host sets before every iteration from the kind of the ply B is
    at: every state word and tree row equal after every iteration over three complete games, the lines equal but for
    A's "full" key."""
    visits, fast, frac = 24, 6, 32768
    a = eh.root_engine(1, visits, weight=0.0, cap=(fast, frac))
    b = eh.root_engine(1, visits, weight=0.0)
    lines_a, lines_b, kinds_seen, inherited_fast = [], [], set(), 0
    for it in range(6000):
        sb = b.game_state(0)
        kind = link.playout_cap_kind(SEED, sb.uid, sb.ply, frac)
        kinds_seen.add(kind)
        inherited_fast += int(sb.phase == 0 and not kind and sb.root_visits >= fast)
        b.set_visits(visits if kind else fast)
        eh.step(a)
        eh.step(b)
        eh.same(eh.dump(a), eh.dump(b))
        lines_a += a.drain_json()
        lines_b += b.drain_json()
        if len(lines_b) >= 3:
            break
    assert len(lines_a) == len(lines_b) >= 3
    assert kinds_seen == {0, 1} and inherited_fast > 0   # (a re-rooted root that already met its fast threshold)
    for uid, (la, lb) in enumerate(zip(lines_a, lines_b)):
        assert b"full" not in lb and _strip_full(la) == lb
        ea = json.loads(la)
        assert list(ea.keys()) == ["boards", "dists", "full", "moves", "result"]
        assert ea["full"] == [link.playout_cap_kind(SEED, uid, p, frac) for p in range(len(ea["moves"]))]
    a.close(), b.close()


@pytest.mark.parametrize("games", [5, 33, 130])
def test_records_say_what_was_searched(games):
    visits, fast, frac = 16, 4, 16384
    net = eh.net()
    e = eh.root_engine(games, visits, weight=0.25, cap=(fast, frac))
    recs, lines = [], []
    for _ in range(40):
        e.run(net, 100, link.DTYPE_BF16)
        e.fetch()
        recs += eh.records3(e.staged_records())
        lines += e.drain_json()
        if {r[0] for r in recs} == set(range(games)):
            break
    assert {r[0] for r in recs} == set(range(games))       # every slot has finished a game
    assert len(lines) == len(recs)
    fulls = fasts = exact = 0
    for slot, uid, result, kind, rows in recs:
        assert kind == 4 and uid % games == slot and result in (1, 2)
        inherited = 0
        for ply, (move, full, counts) in enumerate(rows):
            assert full == link.playout_cap_kind(SEED, uid, ply, frac), (uid, ply)
            T = visits if full else fast
            total = sum(counts.values())
            assert total >= T, (uid, ply, total, T)
            if inherited < T:
                assert total < T + 1, (uid, ply, total, T, inherited)      # K = 1: the move is due at exactly T
                exact += 1
            else:
                assert total == inherited, (uid, ply, total, inherited)  # played after the root's evaluation alone
            # what the next root inherits: every visit of the played edge but the one that created its child
            inherited = max(counts.get(move, 0) - 1, 0)
            fulls += full
            fasts += 1 - full
    assert fulls > 0 and fasts > fulls and exact > 0
    by_key = sorted(json.loads(l)["full"] for l in lines)
    assert by_key == sorted([full for _, full, _ in rows] for _, _, _, _, rows in recs)
    e.close()


def _root_priors(e, g):
    return e.root_report(g, 1)[0].priors.view(np.uint32).copy()


def test_root_noise_on_full_plies_only():
    """The root priors after the root's evaluation at every ply of each slot's first game (uid = slot): on FAST plies
    those of an engine without noise, on FULL plies those of the uncapped engine with noise, at the same uid, ply and
    position (loaded with set_positions: uids restart at the slot numbers), bit for bit."""
    G, visits, fast, frac = 8, 12, 3, 32768
    a = eh.root_engine(G, visits, weight=0.25, cap=(fast, frac))
    plain = eh.root_engine(G, visits, weight=0.0)
    noisy = eh.root_engine(G, visits, weight=0.25)
    checked = {0: 0, 1: 0}
    differ = 0
    for it in range(1500):
        before = [a.game_state(g) for g in range(G)]
        if all(s.uid != g for g, s in enumerate(before)):
            break
        roots = np.array([a.tree(g)[0][0] for g in range(G)], dtype=np.uint64)
        eh.step(a)
        due = [g for g, s in enumerate(before) if s.uid == g and s.phase == 0 and a.game_state(g).phase == 1]
        if not due:
            continue
        plies = np.array([s.ply for s in before], dtype=np.int32)
        for ref in (plain, noisy):
            ref.set_positions(roots, plies)
            eh.step(ref)
        for g in due:
            kind = link.playout_cap_kind(SEED, g, before[g].ply, frac)
            got, p0, p1 = _root_priors(a, g), _root_priors(plain, g), _root_priors(noisy, g)
            assert len(got) == len(p0) == len(p1) > 0
            assert (got == (p1 if kind else p0)).all(), (g, before[g].ply, kind)
            differ += int((p0 != p1).any())
            checked[kind] += 1
    assert checked[0] > 20 and checked[1] > 20 and differ > 40, (checked, differ)
    a.close(), plain.close(), noisy.close()


@pytest.mark.parametrize("K", [4, 8])
def test_leaf_parallel_batches_stop_at_the_plys_own_threshold(K):
    G, visits, fast, frac = 3, 24, 6, 32768
    e = eh.root_engine(G, visits, weight=0.0, cap=(fast, frac), K=K)
    seen = {0: 0, 1: 0}
    truncated = 0
    for it in range(400):
        st = [e.game_state(g) for g in range(G)]
        e.select()
        kind, lb, _ = e.batch_leaves()
        for g, s in enumerate(st):
            filled = int((kind[g] != link.LEAF_NONE).sum())
            if s.phase == 1:
                full = link.playout_cap_kind(SEED, s.uid, s.ply, frac)
                T = visits if full else fast
                want = max(1, min(K, T - s.root_visits))
                assert filled == want and (kind[g, :want] != link.LEAF_NONE).all(), (it, g, filled, want)
                seen[full] += 1
                truncated += int(want < K and not full)
            elif s.phase == 0:
                assert filled == 1 and kind[g, 0] == link.LEAF_ROOT
            else:
                assert filled == 0
        logits, values = helpers.synthetic_evals_distinct(lb.reshape(-1, 2))
        e.set_batch_evals(logits, values)
        e.backup()
    assert seen[0] > 10 and seen[1] > 10 and truncated > 0 and e.stats()["plies"] > 10
    e.close()


def test_device_loop_equals_host_stepping_with_the_cap_on():
    net = eh.net()
    n, G = 200, 33
    a = eh.root_engine(G, 16, weight=0.25, cap=(4, 16384))
    b = eh.root_engine(G, 16, weight=0.25, cap=(4, 16384))
    a.run(net, n, link.DTYPE_BF16)
    a.sync()
    for _ in range(n):
        b.select()
        b.eval(net, link.DTYPE_BF16)
        b.backup()
    eh.same(eh.dump(a), eh.dump(b))
    assert a.stats() == b.stats() and a.stats()["plies"] > 10 * G
    la, lb = a.drain_json(), b.drain_json()
    assert sorted(la) == sorted(lb) and all(b'"full":[' in l for l in la)
    a.close(), b.close()


def test_every_ply_full_and_switched_off_are_the_uncapped_engine():
    net = eh.net(seed=5)
    n, G = 400, 5
    ref = eh.root_engine(G, 12, weight=0.25)
    every = eh.root_engine(G, 12, weight=0.25, cap=(3, 65536))
    off = eh.root_engine(G, 12, weight=0.25, cap=(3, 16384))
    off.set_playout_cap(0, 0)
    for e in (ref, every, off):
        e.run(net, n, link.DTYPE_F32)
        e.sync()
    eh.same(eh.dump(ref), eh.dump(every))
    eh.same(eh.dump(ref), eh.dump(off))
    want = ref.drain_json()
    assert len(want) >= G and not any(b"full" in l for l in want)
    assert off.drain_json() == want                      # byte for byte, no "full" key
    got = every.drain_json()
    assert [_strip_full(l) for l in got] == want
    assert all(set(json.loads(l)["full"]) == {1} for l in got)
    assert ref.stats() == every.stats() == off.stats()
    for e in (ref, every, off):
        e.close()


def test_refusals_leave_the_engine_usable():
    e = eh.root_engine(4, 24, weight=0.0)
    for bad in [(25, 100), (-1, 100), (6, -1), (6, 65537)]:
        with pytest.raises(link.AzhError):
            e.set_playout_cap(*bad)
    eh.step(e)
    e.set_playout_cap(6, 16384)
    with pytest.raises(link.AzhError):
        e.set_visits(5)                       # below fast_visits while the mode is on
    e.set_visits(6)
    e.set_visits(24)
    e.select()
    with pytest.raises(link.AzhError):
        e.set_playout_cap(8, 16384)           # a selected batch awaits its backup
    need, lb = e.leaves()
    e.set_evals(*helpers.synthetic_evals_distinct(lb))
    e.backup()
    e.set_playout_cap(0, 0)
    e.set_visits(5)                           # the mode is off: any value up to the engine's own
    for _ in range(30):
        eh.step(e)
    assert e.stats()["plies"] > 0
    e.close()
    for flags in (link.FLAG_TWO_NETS, link.FLAG_ONE_RANDOM_MOVE):
        r = eh.root_engine(4, 24, weight=0.0, flags=flags)
        with pytest.raises(link.AzhError):
            r.set_playout_cap(6, 16384)
        r.set_playout_cap(0, 0)               # switching off is no request for the mode
        net = eh.net()
        if flags == link.FLAG_TWO_NETS:
            r.run_arena(net, net, 20, link.DTYPE_F32)
        else:
            r.run(net, 20, link.DTYPE_F32)
        r.sync()
        assert r.stats()["steps"] > 0
        r.close()
