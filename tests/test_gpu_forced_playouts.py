"""Forced playouts and policy target pruning on the MI355X (azh_engine_set_forced_playouts): the search in lock step with
the numpy restatement (tests/forced_reference.py) iteration by iteration, the pruned counts of the staged records, the
playout cap's FAST plies left alone, the tie rule, wide roots, the device loop against host stepping, off is off, and the
refusals."""
import numpy as np
import pytest

from ataxxzero_amd import link
from oracle import oracle_lib as orc
from tests import engine_harness as eh
from tests import forced_reference as fr
from tests import helpers
from tests import vl_reference as vlr
from tests.engine_harness import C_PUCT, SEED, WIDE_FEN_BIG, WIDE_FEN_MID

pytestmark = pytest.mark.gpu


def _expected_counts(tree, k):
    """{move: written visits} of the ply played from `tree`, by the restatement"""
    prior, W, n, moves, child = fr.root_arrays(tree)
    m = fr.prune(prior, W, n, k, C_PUCT)
    return {int(mv): int(c) for mv, c, ch in zip(moves, m, child) if ch != vlr.NONE and c != 0}


def _raw_counts(tree):
    prior, W, n, moves, child = fr.root_arrays(tree)
    return {int(mv): int(c) for mv, c, ch in zip(moves, n, child) if ch != vlr.NONE}


def _lock_step(e, k, games, cap=None, tie_first=False, max_iterations=9000):
    """One game slot against the restatement, iteration by iteration, over `games` complete games -> counters.  An
    iteration of the step-wise API is select (a game whose move is due gets no leaf), the due moves, backup and mark: a
    game in phase 1 takes one path, and when the iteration leaves it in phase 2 its move is played by the next one, from the
    tree as it then stands."""
    seen = {"owed": 0, "differs": 0, "marks": 0, "pruned_plies": 0, "fast": 0, "full": 0, "fast_owed_ignored": 0}
    expected = {}    # (uid, ply) -> ({move: written visits}, full)
    done = 0
    for it in range(max_iterations):
        st = e.game_state(0)
        full = 1 if cap is None else link.playout_cap_kind(SEED, st.uid, st.ply, cap[1])
        b = None
        if st.phase == 1:
            pre = e.tree(0)
            b = fr.select(pre, st.root_visits, k, bool(full), C_PUCT, tie_first, 0)
            if not full:
                prior, W, n, _, _ = fr.root_arrays(pre)
                seen["fast_owed_ignored"] += int(fr.owed(prior, n, st.root_visits, k).any())
        values = eh.step(e)[3]
        s2 = e.game_state(0)
        if b is not None:
            assert (s2.uid, s2.ply) == (st.uid, st.ply)
            post = e.tree(0)
            (eb, ei, ee, em), added = vlr.expected_tree(b, values, post)
            assert (eb == post[0]).all() and (ei == post[1]).all() and (ee == post[2]).all() and (em == post[3]).all(), it
            assert s2.root_visits == st.root_visits + added
            seen["owed"] += int(b.forced is not None)
            seen["differs"] += int(b.forced is not None and b.forced != b.puct)
            seen["marks"] += int(eh.root_mark(e) is not None)
        if s2.phase == 2 and st.phase != 2:
            # the move of this ply is due: the next iteration plays it from this tree
            post = e.tree(0)
            want = _expected_counts(post, k) if full else _raw_counts(post)
            seen["pruned_plies"] += int(bool(full) and want != _raw_counts(post))
            expected[(s2.uid, s2.ply)] = (want, full)
        if s2.uid != st.uid:
            e.fetch()
            for slot, uid, result, kind, rows in eh.records3(e.staged_records()):
                assert kind & link.REC_KIND_FORCED and bool(kind & link.REC_KIND_PLAYOUT_CAP) == (cap is not None)
                for ply, (move, fullw, counts) in enumerate(rows):
                    want, f = expected[(uid, ply)]
                    assert counts == want, (uid, ply, f, counts, want)
                    assert cap is None or fullw == f
                    seen["full" if f else "fast"] += 1
                done += 1
            e.drain_json()
            if done >= games:
                break
    assert done >= games
    return seen


def test_lock_step_with_the_restatement():
    e = eh.root_engine(1, 48, weight=0.25, forced=2.0)
    seen = _lock_step(e, 2.0, 3)
    assert seen["owed"] > 0 and seen["differs"] > 0 and seen["pruned_plies"] > 0 and seen["marks"] > 0, seen
    e.close()


def test_lock_step_with_the_playout_cap_on():
    cap = (6, 32768)
    e = eh.root_engine(1, 48, weight=0.25, forced=2.0, cap=cap)
    seen = _lock_step(e, 2.0, 3, cap=cap)
    assert seen["owed"] > 0 and seen["differs"] > 0 and seen["pruned_plies"] > 0, seen
    assert seen["fast"] > 0 and seen["full"] > 0 and seen["fast_owed_ignored"] > 0, seen
    e.close()


def test_lock_step_with_ties_to_the_first_edge():
    e = eh.root_engine(1, 48, weight=0.25, forced=2.0, flags=link.FLAG_TIE_FIRST)
    seen = _lock_step(e, 2.0, 1, tie_first=True)
    assert seen["owed"] > 0 and seen["differs"] > 0, seen
    e.close()


@pytest.mark.parametrize("fen,lo,hi", [(WIDE_FEN_MID, 65, 128), (WIDE_FEN_BIG, 129, 256)])
def test_wide_roots(fen, lo, hi):
    """One ply from a position with more than 64 (two records per lane) and more than 128 (the general level's four) legal
    moves, visits enough that owed edges lie beyond the first record of a lane, in lock step with the restatement."""
    p = orc.pos_from_fen(fen)
    M = len(orc.movegen(p))
    assert lo <= M <= hi
    visits, k = 3 * M, 8.0
    e = eh.root_engine(1, visits, weight=0.25, forced=k, edges_per_node=200)
    e.set_positions(np.array([[int(p.pieces[0]) | (int(p.turn) << 63), int(p.pieces[1])]], dtype=np.uint64),
                    np.zeros(1, dtype=np.int32))
    owed_high = differs = 0
    for it in range(visits + 5):
        st = e.game_state(0)
        if st.phase == 2:
            break
        if st.phase != 1:
            eh.step(e)
            continue
        pre = e.tree(0)
        assert int(pre[1][0, 1]) & 0xFFFF == M
        b = fr.select(pre, st.root_visits, k, True, C_PUCT, False, 0)
        values = eh.step(e)[3]
        post = e.tree(0)
        (eb, ei, ee, em), added = vlr.expected_tree(b, values, post)
        assert (eb == post[0]).all() and (ei == post[1]).all() and (ee == post[2]).all() and (em == post[3]).all(), it
        owed_high += int(b.forced is not None and b.forced >= 64)
        differs += int(b.forced is not None and b.forced != b.puct)
        eh.root_mark(e)
    st = e.game_state(0)
    assert st.phase == 2 and st.root_visits >= visits and owed_high > 0 and differs > 0, (st.as_tuple(), owed_high, differs)
    e.close()


@pytest.mark.parametrize("games", [5, 33, 130])
def test_device_loop_equals_host_stepping(games):
    net = eh.net()
    visits, k, n = 16, 2.0, 600
    a = eh.root_engine(games, visits, weight=0.25, forced=k)
    b = eh.root_engine(games, visits, weight=0.25, forced=k)
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
    assert sorted(a.drain_json()) == sorted(b.drain_json()) and len(ra) == len(rb) > 0
    short = 0
    for slot, uid, result, kind, rows in ra:
        assert kind & link.REC_KIND_FORCED
        for move, full, counts in rows:
            assert counts and all(c >= 1 for c in counts.values())
            assert sum(counts.values()) <= visits      # (every ply is played at `visits` raw visits: an inherited root has fewer)
            short += int(sum(counts.values()) < visits)
    assert short > 0     # some ply wrote fewer visits than its threshold: something was pruned
    a.close(), b.close()


def test_off_is_off():
    ref = eh.root_engine(3, 24, weight=0.25)
    never = eh.root_engine(3, 24, weight=0.25)
    off = eh.root_engine(3, 24, weight=0.25, forced=2.0)
    off.set_forced_playouts(0.0)
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
                assert not r[3] & link.REC_KIND_FORCED
            lines[id(x)] += x.drain_json()
        if len(lines[id(ref)]) >= 3:
            break
    assert len(lines[id(ref)]) >= 3 and lines[id(ref)] == lines[id(never)] == lines[id(off)]
    assert ref.stats() == never.stats() == off.stats()
    # ... and the mode, switched on, does change the search (the comparison above is not vacuous)
    on = eh.root_engine(3, 24, weight=0.25, forced=2.0)
    ref2 = eh.root_engine(3, 24, weight=0.25)
    differ = False
    for it in range(200):
        eh.step(on), eh.step(ref2)
        differ = differ or any((x.shape != y.shape or (x != y).any()) for g in range(3) for x, y in zip(on.tree(g), ref2.tree(g)))
    assert differ
    for x in (ref, never, off, on, ref2):
        x.close()


def test_refusals_leave_the_engine_usable():
    e = eh.root_engine(4, 24, weight=0.25)
    for bad in (-1.0, float("nan")):
        with pytest.raises(link.AzhError):
            e.set_forced_playouts(bad)
    eh.step(e)
    e.select()
    with pytest.raises(link.AzhError):
        e.set_forced_playouts(2.0)            # a selected batch awaits its backup
    need, lb = e.leaves()
    e.set_evals(*helpers.synthetic_evals_distinct(lb))
    e.backup()
    e.set_forced_playouts(2.0)
    with pytest.raises(link.AzhError):
        e.set_leaf_batch(4, 1)                # K > 1 while the mode is on
    with pytest.raises(link.AzhError):
        e.set_solver(True)
    e.set_leaf_batch(1, 1)                    # K = 1 without the solver is the one-leaf search: no request
    for _ in range(40):
        eh.step(e)
    assert e.stats()["plies"] > 0
    e.set_forced_playouts(0.0)
    e.set_leaf_batch(4, 1)
    with pytest.raises(link.AzhError):
        e.set_forced_playouts(2.0)            # ... and the other way round
    e.set_leaf_batch(1, 1)
    e.set_solver(True)
    with pytest.raises(link.AzhError):
        e.set_forced_playouts(2.0)
    e.set_solver(False)
    e.set_forced_playouts(2.0)
    for _ in range(30):
        eh.step(e)
    e.close()
    for flags in (link.FLAG_TWO_NETS, link.FLAG_ONE_RANDOM_MOVE):
        r = eh.root_engine(4, 24, weight=0.0, flags=flags)
        with pytest.raises(link.AzhError):
            r.set_forced_playouts(2.0)
        r.set_forced_playouts(0.0)            # switching off is no request for the mode
        net = eh.net()
        if flags == link.FLAG_TWO_NETS:
            r.run_arena(net, net, 20, link.DTYPE_F32)
        else:
            r.run(net, 20, link.DTYPE_F32)
        r.sync()
        assert r.stats()["steps"] > 0
        r.close()
