"""Search settings per side on the MI355X (azh_engine_set_search_sets): every iteration of the HIP engine equals the numpy
restatement of the leaf-parallel search (tests/exploration_reference.py) called with the set of the root's mover — across
plies, game ends and restarts, with the solver off and on — one set equal to the engine's settings changes nothing, a move
named by the host and a loaded position are searched with the new mover's set, the device loop equals host stepping, the
device's tally equals the table recounted from the records, every cell of the mode table's tenth row refuses in the table's
words, and tools/settings_match.py runs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import link, model
from tests import engine_harness as eh
from tests import helpers
from tests import leaf_lockstep as lls
from tests import solver_reference as sr

pytestmark = pytest.mark.gpu

ROOT = helpers.ROOT
# two sets that differ in every field at once, and a third between them
A = dict(visits=24, leaves=1, virtual_loss=1, c_puct=1.0, fpu_reduction=-1.0, c_base=0.0, c_init=0.0)
B = dict(visits=40, leaves=7, virtual_loss=3, c_puct=2.5, fpu_reduction=0.25, c_base=19652.0, c_init=1.25)
C = dict(visits=32, leaves=4, virtual_loss=2, c_puct=1.75, fpu_reduction=0.5, c_base=0.0, c_init=0.0)
B64 = dict(B, leaves=64, virtual_loss=2)
VISITS = 48      # the engines' own threshold: above every set's, so a move that came due at it would show


def _config(G, flags, blockers=0, visits=VISITS, seed=11, max_plies=400, **more):
    return lls.config(G, flags, blockers, visits, seed, max_plies, **more)


def _engine(G, K, flags, blockers, sets, family="late", solver=False, max_plies=400, visits=VISITS, seed=11, vl=1):
    return lls.engine(G, flags, blockers, visits, seed, max_plies, start=family, leaf_batch=(K, vl) if K > 1 else None,
                      solver=solver, sets=sets)


def _f32(t):
    return {k: (float(np.float32(v)) if isinstance(v, float) else v) for k, v in t.items()}


def _turn(tree):
    return int(tree[0][0][0]) >> 63


class Met:
    """The lock step of tests/leaf_lockstep.py with the set of the root's mover as the settings in force, and what its
    iterations met: what every test below that steps an engine uses."""

    def __init__(self, e, cfg, sets, solver=False):
        self.sets = sets
        self.ls = lls.LockStep(e, cfg, solver=solver, settings=lambda g, tree, state: sets[self.set_of(tree, state.uid)])
        self.seen = {"differs": 0, "batches": 0, "proven": 0, "roots": 0, "due": 0}
        self.used = set()                            # set indices used at a root
        self.plies = [set() for _ in range(e.G)]     # (uid, ply) whose root was searched, per slot
        self.last_set = [None] * e.G                 # the set index of the slot's last batch

    def set_of(self, tree, uid, other=False):
        return link.search_set_pairing(uid, len(self.sets))[_turn(tree) ^ int(other)]

    def iteration(self):
        rec = self.ls.step()
        for g, r in rec.games.items():
            i, j = self.set_of(r.pre, r.state.uid), self.set_of(r.pre, r.state.uid, other=True)
            self.used.add(i)
            self.plies[g].add((r.state.uid, r.state.ply))
            self.last_set[g] = i
            self.seen["batches"] += 1
            self.seen["proven"] += len(r.proven)
            self.seen["due"] += int(r.due)
            # a level where the game's two sets pick different edges: the first path under each set's scoring alone
            if j != i:
                one = dict(visits=r.settings["visits"], leaves=1, virtual_loss=1)
                mine = self.ls.select(r.pre, r.state.root_visits, dict(r.settings, **one))
                other = self.ls.select(r.pre, r.state.root_visits, dict(self.sets[j], **one))
                self.seen["differs"] += int(mine.paths != other.paths)
        self.seen["roots"] += sum(1 for st in rec.states if st.phase == 0)


# (G, engine K, blockers, flags, sets, family, solver, max_plies): max_plies cuts the games short, so that every slot begins
# its second game — another uid, another pairing — within a few dozen iterations
CASES = {
    "G1K1": (1, 1, 0, 0, [A, dict(B, leaves=1)], "late", False, 13),
    "G5K7-block4": (5, 7, helpers.BLOCK4_MASK, 0, [A, B], "late", False, 13),
    "G5K7-block4-noreuse": (5, 7, helpers.BLOCK4_MASK, link.FLAG_NO_REUSE | link.FLAG_TIE_FIRST, [A, B], "late", False, 13),
    "G5K64-start": (5, 64, 0, 0, [A, B64], "start", False, 3),
    "G4K7-three-sets": (4, 7, 0, 0, [A, B, C], "late", False, 13),
    "G5K7-block4-solver": (5, 7, helpers.BLOCK4_MASK, 0, [A, B], "late", True, 13),
}
_RESULTS = {}


def _case(name):
    return lls.memo(_RESULTS, name, lambda: _run_case(*CASES[name]))


def _run_case(G, K, blockers, flags, sets, family, solver, max_plies, limit=400):
    e, cfg = _engine(G, K, flags, blockers, sets, family, solver, max_plies)
    assert e.search_sets() == [_f32(t) for t in sets]
    ls = Met(e, cfg, sets, solver)
    for _ in range(limit):
        ls.iteration()
        second = [any(uid >= G for uid, _ in p) for p in ls.plies]
        if all(second) and all(len(p) >= 4 for p in ls.plies):
            break
    assert all(second) and all(len(p) >= 4 for p in ls.plies), ls.plies      # >= 3 plies, and into the second game
    e.close()
    return ls


@pytest.mark.parametrize("name", list(CASES))
def test_every_iteration_equals_the_restatement_with_the_movers_set(name):
    ls = _case(name)
    assert ls.used == set(range(len(CASES[name][4]))), ls.used            # every set was used at a root
    assert ls.seen["due"] >= 3 * CASES[name][0] and ls.seen["roots"] > 0


def test_the_cases_met_levels_where_the_sets_differ_and_proofs():
    for name in CASES:
        if name != "G1K1":
            assert _case(name).seen["differs"] > 0, name
    assert sum(_case(name).seen["differs"] for name in CASES) > 0
    assert _case("G5K7-block4-solver").seen["proven"] > 0


def test_a_slots_second_game_has_another_pairing():
    """(G odd: uid g + G has the other parity, so the colours swap; the lock step above follows the slot's word through it)"""
    for g in range(5):
        assert link.search_set_pairing(g, 2) != link.search_set_pairing(g + 5, 2)


# ------------------------------------------------------------------ identity


def _records(e):
    return [(r.slot, r.uid, r.result, r.kind, r.plies) for r in link.records(eh.staged(e), markers=True)]


def test_one_set_equal_to_the_engines_settings_changes_nothing():
    K, VL = 4, 2
    own = dict(visits=VISITS, leaves=K, virtual_loss=VL, c_puct=1.0, fpu_reduction=-1.0, c_base=0.0, c_init=0.0)
    a, _ = _engine(3, K, 0, 0, [own], max_plies=14, vl=VL)
    b, _ = _engine(3, K, 0, 0, None, max_plies=14, vl=VL)
    assert a.search_sets() == [_f32(own)] and b.search_sets() == []
    for _ in range(90):
        eh.step(a, K=K), eh.step(b, K=K)
    eh.same(eh.dump(a, raw=True), eh.dump(b, raw=True))
    assert a.stats() == b.stats() and a.stats()["plies"] >= 9
    assert _records(a) == _records(b)
    # off again: the engine that never had them
    a.set_search_sets([])
    assert a.search_sets() == [] and a.search_set_stats().shape == (0, 0, 4)
    for _ in range(30):
        eh.step(a, K=K), eh.step(b, K=K)
    eh.same(eh.dump(a, raw=True), eh.dump(b, raw=True))
    assert a.stats() == b.stats() and _records(a) == _records(b)
    a.close(), b.close()


# ------------------------------------------------------------------ host moves and loaded positions


@pytest.mark.parametrize("flags,status", [(0, link.PLAY_KEPT), (link.FLAG_NO_REUSE, link.PLAY_FRESH)], ids=["kept", "fresh"])
def test_after_a_host_move_the_new_movers_set_searches(flags, status):
    G, K = 2, 7
    e, cfg = _engine(G, K, flags, 0, [A, B], family="start")      # (from the start position: no move ends the game)
    ls = Met(e, cfg, [A, B])
    for _ in range(6):
        ls.iteration()
    before = list(ls.last_set)
    assert None not in before
    moves = np.zeros(G, dtype=np.uint16)
    for g in range(G):
        boards, info, edges, mv = e.tree(g)
        first, M = int(info[0][0]), int(info[0][1]) & 0xFFFF
        j = int(np.argmax(edges[first:first + M, 1]))          # a visited edge: it has a child
        moves[g] = mv[first + j]
    assert list(e.play_moves(moves)) == [status] * G
    turns = [_turn(e.tree(g)) for g in range(G)]
    for _ in range(4):
        ls.iteration()
    for g in range(G):
        assert ls.last_set[g] == link.search_set_pairing(g, 2)[turns[g]] != before[g]
    e.close()


def test_a_loaded_position_with_o_to_move_is_searched_with_os_set():
    G, K = 2, 7
    e, cfg = _engine(G, K, 0, 0, [A, B], family="start")
    boards = [(w0, w1) for w0, w1, bl in sr.late_positions(10) if bl == 0 and w0 >> 63][:G]
    assert len(boards) == G
    e.set_positions(np.array(boards, dtype=np.uint64), np.full(G, 11, np.int32))
    ls = Met(e, cfg, [A, B])
    for _ in range(4):
        ls.iteration()
    assert ls.last_set == [link.search_set_pairing(g, 2)[1] for g in range(G)]
    e.close()


# ------------------------------------------------------------------ the device loop


@pytest.mark.parametrize("K,dtype", [(1, link.DTYPE_F32), (7, link.DTYPE_F16)])
def test_device_loop_equals_host_stepping_across_re_roots_and_game_ends(K, dtype):
    net = eh.net(2)
    sets = [A, dict(B, leaves=min(K, 7)), dict(C, leaves=min(K, 4))]
    n = 260 if K == 1 else 90
    a, _ = _engine(3, K, 0, 0, sets, max_plies=14)
    b, _ = _engine(3, K, 0, 0, sets, max_plies=14)
    a.run(net, n, dtype)
    a.sync()
    for _ in range(n):
        b.select()
        b.eval(net, dtype)
        b.backup()
    eh.same(eh.dump(a, raw=True), eh.dump(b, raw=True))
    assert a.stats() == b.stats() and a.stats()["plies"] > 6
    assert a.stats()["games"] + a.stats()["dropped"] >= 3                   # games ended inside the loop
    assert (a.search_set_stats() == b.search_set_stats()).all() and a.search_set_stats()[:, :, 0].sum() >= 3
    assert _records(a) == _records(b)
    a.close(), b.close()


# ------------------------------------------------------------------ the tally

SMALL = [dict(A, visits=8), dict(B, visits=12, leaves=4), dict(C, visits=10)]


def _recount(words, n):
    table = np.zeros((n, n, 4), dtype=np.uint64)
    for r in link.records(words, markers=True):
        x, o = link.search_set_pairing(r.uid, n)
        dropped = r.kind & link.REC_KIND_MASK == link.REC_KIND_DROPPED
        table[x, o, link.SET_STAT_GAMES] += 1
        table[x, o, link.SET_STAT_UNDECIDED if dropped or r.result == 0 else r.result] += 1
    return table


@pytest.mark.parametrize("max_plies", [400, 2], ids=["played-out", "cut-at-the-ply-limit"])
def test_the_tally_equals_the_table_recounted_from_the_records(max_plies):
    G, limit, n = 6, 24, 3
    net = eh.net(1)
    cfg = _config(G, link.FLAG_NO_REUSE | link.FLAG_TIE_FIRST, visits=16, max_plies=max_plies)
    e = link.Engine(cfg)
    late = [(int(w0) & ~(1 << 63), int(w1), 0, int(w0) >> 63) for w0, w1, bl in sr.late_positions(8) if bl == 0]
    assert len(late) >= 4
    e.set_start_pool(late[-12:], stride=2)      # (eight empty cells: a game lasts longer than two plies, and not long)
    e.set_leaf_batch(4, 1)
    e.set_search_sets(SMALL)
    e.set_game_limit(limit)
    assert (e.search_set_stats() == 0).all()
    words = []
    for _ in range(40):
        e.run(net, 60, link.DTYPE_F16)
        words.append(eh.staged(e))
        st = e.stats()
        if st["games"] + st["dropped"] == limit:
            break
    st = e.stats()
    assert st["games"] + st["dropped"] == limit and st["ring_overflow"] == 0
    table = e.search_set_stats()
    assert table.shape == (n, n, 4)
    assert (table == _recount(np.concatenate(words), n)).all(), table
    assert int(table[:, :, link.SET_STAT_GAMES].sum()) == limit
    assert (table[:, :, 0] == table[:, :, 1] + table[:, :, 2] + table[:, :, 3]).all()
    assert all(table[i, i, 0] == 0 for i in range(n))
    assert (table[:, :, 0][~np.eye(n, dtype=bool)] == limit // (n * (n - 1))).all()      # every ordered pair equally often
    assert int(table[:, :, link.SET_STAT_UNDECIDED].sum()) == st["dropped"]
    if max_plies == 2:
        assert st["dropped"] > 0
    else:
        assert st["games"] > 0
    # setting the sets again zeroes the tally
    e.set_search_sets(SMALL[:2])
    assert e.search_set_stats().shape == (2, 2, 4) and (e.search_set_stats() == 0).all()
    e.close()


# ------------------------------------------------------------------ refusals: the tenth row of the mode table

SETTER = "azh_engine_set_search_sets"
PHRASE = "search settings per side (azh_engine_set_search_sets)"
UAI = link.FLAG_NO_REUSE | link.FLAG_TIE_FIRST


@pytest.mark.parametrize("kwargs,cause", [(dict(flags=UAI | link.FLAG_TWO_NETS), "AZH_FLAG_TWO_NETS"),
                                          (dict(flags=UAI | link.FLAG_ONE_RANDOM_MOVE), "AZH_FLAG_ONE_RANDOM_MOVE"),
                                          (dict(flags=UAI | link.FLAG_EVAL_CACHE), "AZH_FLAG_EVAL_CACHE"),
                                          (dict(flags=UAI | link.FLAG_SYMMETRY_AVG), "AZH_FLAG_SYMMETRY_AVG"),
                                          (dict(flags=UAI, select_budget=4), "select_budget > 0")])
def test_every_create_time_cause(kwargs, cause):
    e = link.Engine(_config(4, kwargs.pop("flags"), seed=7, **kwargs))
    lls.refused(lambda: e.set_search_sets([A, dict(B, leaves=1)]), -4, "%s: not supported with %s" % (SETTER, cause))
    assert e.search_sets() == []
    e.set_search_sets([])          # switching off is no request for the mode
    e.close()


OTHERS = {
    "gumbel": ("azh_engine_set_gumbel", lambda e: e.set_gumbel(4), lambda e: e.set_gumbel(0),
               "the Gumbel root search (azh_engine_set_gumbel)"),
    "forced": ("azh_engine_set_forced_playouts", lambda e: e.set_forced_playouts(2.0), lambda e: e.set_forced_playouts(0.0),
               "forced playouts (azh_engine_set_forced_playouts)"),
    "cap": ("azh_engine_set_playout_cap", lambda e: e.set_playout_cap(8, 16384), lambda e: e.set_playout_cap(0, 0),
            "the playout cap (azh_engine_set_playout_cap)"),
    "exploration": ("azh_engine_set_exploration", lambda e: e.set_exploration(0.25, 0.0, 0.0),
                    lambda e: e.set_exploration(-1.0, 0.0, 0.0),
                    "first-play urgency or a growing exploration rate (azh_engine_set_exploration)"),
}


@pytest.mark.parametrize("other", list(OTHERS))
def test_the_excluded_modes_in_both_orders(other):
    setter, on, off, phrase = OTHERS[other]
    sets = [A, dict(B, leaves=1)]
    e = link.Engine(_config(4, UAI, seed=7))
    on(e)
    lls.refused(lambda: e.set_search_sets(sets), -4, "%s: not supported with %s" % (SETTER, phrase))
    assert e.search_sets() == []
    off(e)
    e.set_search_sets(sets)
    lls.refused(lambda: on(e), -4, "%s: not supported with %s" % (setter, PHRASE))
    e.set_search_sets([])
    on(e)
    off(e)
    e.close()


def test_it_composes_with_the_other_modes():
    e = link.Engine(_config(4, UAI, seed=7))
    e.set_leaf_batch(4, 2)
    e.set_search_sets([A, dict(B, leaves=4)])
    e.set_solver(True)
    e.set_temperature(np.ones(400, dtype=np.float32), None)
    e.set_resign(0.1, 2, 0)
    e.set_random_symmetry(True)
    e.set_game_limit(8)
    for _ in range(40):
        eh.step(e, K=4)
    assert e.stats()["plies"] > 0
    e.close()


def test_bad_arguments_a_selected_batch_and_an_unchanged_engine():
    sets = [A, dict(B, leaves=4)]
    e = link.Engine(_config(4, UAI, seed=7))
    twin = link.Engine(_config(4, UAI, seed=7))
    for x in (e, twin):
        x.set_leaf_batch(4, 2)
        x.set_search_sets(sets)
    inf, nan = float("inf"), float("nan")
    bad = [("visits", 0, "need 1 <= visits <= 48 (the engine's)"), ("visits", 49, "need 1 <= visits <= 48 (the engine's)"),
           ("leaves", 0, "need 1 <= leaves <= 4 (azh_engine_set_leaf_batch)"),
           ("leaves", 5, "need 1 <= leaves <= 4 (azh_engine_set_leaf_batch)"),
           ("virtual_loss", 0, "need 1 <= virtual_loss <= 16"), ("virtual_loss", 17, "need 1 <= virtual_loss <= 16"),
           ("c_puct", -0.5, "need a finite c_puct >= 0"), ("c_puct", nan, "need a finite c_puct >= 0"),
           ("c_puct", inf, "need a finite c_puct >= 0")]
    bad += [(k, v, "need finite arguments, c_base >= 0 and c_init >= 0")
            for k, v in (("fpu_reduction", nan), ("fpu_reduction", inf), ("c_base", nan), ("c_base", -1.0), ("c_base", inf),
                         ("c_init", nan), ("c_init", -0.5), ("c_init", inf))]
    for field, value, why in bad:
        for at in (0, 1):           # the first offending set is the one named
            rows = [dict(t) for t in sets]
            rows[1][field] = value
            rows[at][field] = value
            lls.refused(lambda: e.set_search_sets(rows), -2, "%s: set %d: %s" % (SETTER, at, why))
            assert e.search_sets() == [_f32(t) for t in sets]
    lls.refused(lambda: e.set_search_sets([A] * 17), -2, SETTER + ": need 0 <= n <= 16")
    # the engine's visits and K may not go below a set's
    lls.refused(lambda: e.set_visits(39), -2, "azh_engine_set_visits: 39 is below the visits 40 of search set 1")
    lls.refused(lambda: e.set_leaf_batch(3, 2), -2, "azh_engine_set_leaf_batch: 3 is below the leaves 4 of search set 1")
    e.set_visits(40), twin.set_visits(40)
    # a selected batch awaits its backup: requests and switching off alike, and a bad argument is still -2
    e.select()
    kind, lb, _ = e.batch_leaves()
    for rows in ([dict(B, leaves=4), A], []):
        lls.refused(lambda: e.set_search_sets(rows), -3, SETTER + ": a selected batch awaits its backup")
        assert e.search_sets() == [_f32(t) for t in sets]
    lls.refused(lambda: e.set_search_sets([dict(A, visits=0)]), -2, SETTER + ": set 0: need 1 <= visits <= 40 (the engine's)")
    e.set_batch_evals(*helpers.synthetic_evals_distinct(lb.reshape(-1, 2)))
    e.backup()
    eh.step(twin, K=4)
    # every refused call left the sets, the tally and the coming batches as they were
    for _ in range(60):
        eh.step(e, K=4), eh.step(twin, K=4)
    eh.same(eh.dump(e, raw=True), eh.dump(twin, raw=True))
    assert e.stats() == twin.stats() and e.stats()["plies"] > 0
    assert (e.search_set_stats() == twin.search_set_stats()).all()
    e.close(), twin.close()


def test_the_header_holds_the_row():
    with open(os.path.join(ROOT, "include", "ataxxzero_hip.h")) as f:
        text = " ".join(f.read().replace(" *", " ").split())
    assert "Ten modes" in text
    assert ("search sets n != 0 TWO_NETS, ONE_RANDOM_MOVE, EVAL_CACHE, SYMMETRY_AVG; Gumbel, forced playouts, select_budget > 0 "
            "playout cap, exploration") in text
    assert '"search settings per side (azh_engine_set_search_sets)"' in text


# ------------------------------------------------------------------ the tool


def test_the_match_tool_plays_a_table(tmp_path):
    conv, bn = model.random_init(1, 128, seed=5, perturb_bn=True)
    net = str(tmp_path / "net.npy")
    model.save_model(net, conv, bn)
    out = str(tmp_path / "table.txt")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "settings_match.py"), "--network", net, "--games", "12", "--concurrent", "6",
           "--opening-plies", "2", "--set", "visits=8", "--set", "visits=12,leaves=4,vl=2,cpuct=2.5,fpu=0.25",
           "--set", "visits=10,cpuct-base=19652,cpuct-init=1.25", "--out", out]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ))
    assert res.returncode == 0, res.stderr[-2000:]
    with open(out) as f:
        rows = [l.split() for l in f.read().splitlines() if re.match(r"\s*\d+-\d+\s", l)]
    assert [r[0] for r in rows] == ["0-1", "0-2", "1-2"]
    assert sum(int(r[1]) for r in rows) == 12
    for r in rows:
        assert int(r[1]) == 4 == sum(int(v) for v in r[2:7])
