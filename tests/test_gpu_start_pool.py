"""A start position and wall map per game, drawn from a pool (azh_engine_set_start_pool): the tower and the feature kernel with a
mask per board; the pooled engine against the CPU oracle, record by record and uid by uid, through the step-wise API and the
device-resident loop; the modes the oracle does not know against single-start device engines; the refusals; the command lines.
Maps and shared pieces: tests/start_pool_fixtures.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import arena, link, model
from oracle import oracle_lib as orc
from tests import engine_harness as eh
from tests import fresh_process, helpers
from tests import start_pool_fixtures as spf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = link.DTYPE_F32, link.DTYPE_BF16, link.DTYPE_F16


# ------------------------------------------------------------------ the tower and the feature kernel

def _seven_boards():
    """7 boards — two full three-board tiles and a partial one — with a mask each, drawn from {0, default, asymmetric}"""
    pool = spf.entries()
    boards = np.array([b for b, _, _ in helpers.fixture_positions(40)[3:40:5]][:7], dtype=np.uint64)
    boards[:, 0] &= np.uint64((1 << 63) - 1)
    assert boards.shape == (7, 2)
    masks = np.array([pool[i][2] for i in (0, 1, 2, 2, 0, 1, 1)], dtype=np.uint64)
    return boards, masks


@pytest.mark.parametrize("thin", [False, True], ids=["three-board", "thin"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_tower_with_a_mask_per_board_equals_a_launch_per_mask(dtype, thin):
    net = eh.net()
    boards, masks = _seven_boards()
    logits, values = net.forward(boards, masks, dtype, thin=thin)
    for m in sorted(set(int(v) for v in masks)):
        want_l, want_v = net.forward(boards, m, dtype, thin=thin)      # the same 7 boards in the same order: a board keeps its slot
        rows = masks == np.uint64(m)
        assert rows.any() and (logits[rows].view(np.uint32) == want_l[rows].view(np.uint32)).all(), hex(m)
        assert (values[rows].view(np.uint32) == want_v[rows].view(np.uint32)).all(), hex(m)
        other_l, _ = net.forward(boards, int(masks[~rows][0]), dtype, thin=thin)
        assert (logits[rows] != other_l[rows]).any()                   # (the mask matters to these rows)


def test_symmetry_averaged_tower_with_a_mask_per_board():
    net = eh.net()
    boards, masks = _seven_boards()
    logits, values = net.forward_sym(boards, masks, F32)
    for m in sorted(set(int(v) for v in masks)):
        want_l, want_v = net.forward_sym(boards, m, F32)
        rows = masks == np.uint64(m)
        assert (logits[rows].view(np.uint32) == want_l[rows].view(np.uint32)).all(), hex(m)
        assert (values[rows].view(np.uint32) == want_v[rows].view(np.uint32)).all(), hex(m)


@pytest.mark.parametrize("mode,thin", [(link.FORWARD_PLAIN, False), (link.FORWARD_THIN, True), (link.FORWARD_SYM, None)],
                         ids=["plain", "thin", "sym"])
def test_tower_without_a_mask_array_gives_the_bytes_of_the_plain_forward(mode, thin):
    """azh_net_forward in its three modes with a null mask array"""
    net = eh.net()
    boards, _ = _seven_boards()
    logits = np.zeros((7, 7, 7, 17), np.float32)
    values = np.zeros((7, 1), np.float32)
    link.check(link.load().azh_net_forward(net.h, BF16, mode, 7, boards.ctypes.data, 0, None, logits.ctypes.data, values.ctypes.data))
    want_l, want_v = net.forward_sym(boards, 0, BF16) if thin is None else net.forward(boards, 0, BF16, thin=thin)
    assert logits.tobytes() == want_l.tobytes() and values.tobytes() == want_v.tobytes()
    bad = np.array([0, 0, 1 << 49, 0, 0, 0, 0], dtype=np.uint64)
    with pytest.raises(link.AzhError) as err:
        link.check(link.load().azh_net_forward(net.h, BF16, mode, 7, boards.ctypes.data, 0, bad.ctypes.data, logits.ctypes.data,
                                               values.ctypes.data))
    assert "board 2" in str(err.value)


def test_leaf_features_carry_the_walls_of_each_leaf_s_game():
    pool = spf.entries()
    e = spf.pooled_engine(pool, 6, 8)
    seen = set()
    for _ in range(12):
        n = e.select()
        need, lb = e.leaves()
        rows, games = e.leaf_features(n)
        assert n == int((need != 0).sum()) and len(games) == n
        for row, g in zip(rows, games):
            walls = e.uid_blockers(e.game_state(int(g)).uid)
            assert walls == pool[e.game_state(int(g)).uid % 4][2]
            assert (row == link.features_batch(lb[int(g)][None, :], walls)[0]).all(), int(g)
            seen.add(walls)
        logits, values = helpers.synthetic_evals_distinct(lb)
        e.set_evals(logits, values)
        e.backup()
    assert len(seen) == 4


# ------------------------------------------------------------------ the pooled engine against the oracle

G, VISITS = 6, 8


def _collect(e, found, advance, rounds=400):
    """runs `advance` and gathers the staged records until every slot has finished at least two games"""
    for _ in range(rounds):
        advance()
        found.update(spf.device_records(eh.staged(e)))
        if all(sum(1 for u in found if u % e.G == g) >= 2 for g in range(e.G)):
            return
    raise AssertionError("the slots did not finish two games each: %r" % sorted(found))


def _consecutive_games_on_different_masks(found, pool, games):
    return any(u + games in found and pool[u % len(pool)][2] != pool[(u + games) % len(pool)][2] for u in found)


def test_step_wise_search_on_a_pool_equals_the_oracle_of_each_entry():
    pool = spf.entries()
    e = spf.pooled_engine(pool, G, VISITS)
    found = {}
    _collect(e, found, lambda: [eh.step(e) for _ in range(40)])
    assert _consecutive_games_on_different_masks(found, pool, G)
    spf.never_on_a_wall(found, pool)
    spf.check_against_oracle(found, pool, G, VISITS, lambda entry: helpers.synthetic_evals_distinct)
    assert e.stats()["ring_overflow"] == 0 and e.stats()["edge_overflow"] == 0


def _net_evaluator(net):
    def of(entry):
        def evaluate(lb):
            logits, values = net.forward(lb, entry[2], F32)
            return logits.reshape(len(lb), 833), values.reshape(-1)
        return evaluate
    return of


@pytest.mark.parametrize("flags", [0, link.FLAG_EVAL_CACHE], ids=["plain", "eval-cache"])
def test_device_loop_on_a_pool_equals_the_oracle_of_each_entry(flags):
    pool, net = spf.entries(), eh.net()
    e = spf.pooled_engine(pool, G, VISITS, flags=flags)
    found = {}
    _collect(e, found, lambda: e.run(net, 60, F32))
    assert _consecutive_games_on_different_masks(found, pool, G)          # at least one restart per slot, onto another mask
    spf.never_on_a_wall(found, pool)
    spf.check_against_oracle(found, pool, G, VISITS, _net_evaluator(net), flags=flags)


def test_two_pooled_engines_in_one_run_equal_the_oracle_of_each_entry():
    pool, net = spf.entries(), eh.net()
    seeds = (spf.SEED, spf.SEED + 1000003)
    engines = [spf.pooled_engine(pool, G, VISITS, seed=s) for s in seeds]
    found = [{}, {}]

    def advance():
        link.run_engines(engines, net, 60, F32)
    for e, f in zip(engines, found):
        _collect(e, f, advance)
    for s, f in zip(seeds, found):
        assert _consecutive_games_on_different_masks(f, pool, G)
        spf.check_against_oracle(f, pool, G, VISITS, _net_evaluator(net), seed=s)
    assert found[0] != found[1]


# ------------------------------------------------------------------ modes the oracle does not know: against single-start engines

def _by_slot(e):
    out = {}
    for r in link.records(eh.staged(e)):
        out.setdefault(r.slot, []).append((r.uid, r.result, r.kind, r.plies))
    return out


def _pool_equals_singles(pool, stride, make, advance, games=4, rounds=3):
    """the pooled engine's slots equal, slot for slot, the slots of the single-start engines of their entries: trees and records"""
    pooled = make(pool[0])
    pooled.set_start_pool(pool, stride)
    singles = [make(entry) for entry in pool]
    finished = 0
    for _ in range(rounds):
        for e in [pooled] + singles:
            advance(e)
        recs = [_by_slot(e) for e in [pooled] + singles]
        for g in range(games):
            k = link.start_pool_entry(g, len(pool), stride)
            assert link.start_pool_entry(g + games, len(pool), stride) == k           # (the slot's entry is fixed)
            eh.same(eh.dump(pooled, [g]), eh.dump(singles[k], [g]))
            assert recs[0].get(g, []) == recs[1 + k].get(g, []), g
            finished += len(recs[0].get(g, []))
    assert finished >= games, finished                                                # (games ended, and slots restarted)
    return pooled


MODES = {
    "leaf-batch": (0, 0.25, lambda e: e.set_leaf_batch(4, 1)),
    "solver": (0, 0.25, lambda e: e.set_solver(True)),
    "gumbel": (link.FLAG_NO_REUSE, 0.0, lambda e: e.set_gumbel(4, 50.0, 1.0)),
    "random-symmetry": (0, 0.25, lambda e: e.set_random_symmetry(True)),
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_modes_on_a_pool_equal_single_start_engines(mode):
    flags, weight, switch = MODES[mode]
    entries, net = spf.entries(), eh.net()
    pool = [entries[0], entries[1]] if mode == "random-symmetry" else [entries[2], entries[1]]   # (two invariant masks there)

    def make(entry):
        e = spf.device_engine(entry, 4, VISITS, flags=flags, weight=weight)
        return e

    def advance(e):
        if not getattr(e, "_switched", False):
            switch(e)                                                   # (after the pool is set: the order a caller uses)
            e._switched = True
        e.run(net, 600, F32)
        e.sync()
    _pool_equals_singles(pool, 1, make, advance)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16-pair-launch"])
def test_two_net_arena_with_stride_two_shares_a_map_per_pairing(dtype):
    entries = spf.entries()
    pool = [entries[2], entries[1]]
    net_a, net_b = eh.net(), eh.net(seed=4)

    def advance(e):
        e.run_arena(net_a, net_b, 600, dtype)
        e.sync()
    pooled = _pool_equals_singles(pool, 2, lambda entry: spf.device_engine(entry, 4, VISITS, flags=link.FLAG_ARENA, weight=0.0),
                                  advance)
    assert [pooled.uid_blockers(u) for u in range(8)] == [pool[k][2] for k in (0, 0, 1, 1, 0, 0, 1, 1)]


def test_a_pool_of_identical_entries_is_the_engine_created_with_that_start():
    entry, net = spf.entries()[1], eh.net()
    plain = spf.device_engine(entry, 5, VISITS)
    pooled = spf.pooled_engine([entry] * 3, 5, VISITS)
    for _ in range(2):
        for e in (plain, pooled):
            e.run(net, 200, F32)
            e.sync()
        eh.same(eh.dump(plain, raw=True), eh.dump(pooled, raw=True))
        # (two games that end in one iteration reach the ring in either order: the records are compared by uid)
        ra, rb = (sorted(eh.records(eh.staged(e)), key=lambda r: r[1]) for e in (plain, pooled))
        assert len(ra) > 0 and ra == rb
    assert plain.stats() == pooled.stats()


def test_taking_the_pool_away_restores_the_configured_start():
    pool = spf.entries()
    plain = spf.device_engine(pool[0], 4, VISITS)
    e = spf.device_engine(pool[0], 4, VISITS)
    e.set_start_pool(pool[1:])
    assert e.tree(0)[0][0].tolist() != plain.tree(0)[0][0].tolist() and e.uid_blockers(3) == pool[1][2]
    e.set_start_pool([])
    eh.same(eh.dump(plain), eh.dump(e))
    assert e.uid_blockers(3) == pool[0][2]


# ------------------------------------------------------------------ refusals

def _refused(e, call, code_words):
    before = eh.dump(e, raw=True)
    with pytest.raises(link.AzhError) as err:
        call()
    assert code_words in str(err.value), str(err.value)
    eh.same(before, eh.dump(e, raw=True))
    return str(err.value)


def test_refusals_leave_the_engine_as_it_was_and_playing():
    pool = spf.entries()
    x, o, walls, turn = pool[2]
    lone_x, lone_o = x & -x, o & -o
    full = spf.BOARD & ~(x | o)
    e = spf.pooled_engine(pool[:2], 4, VISITS)
    bad = {
        "a cell holds stones of both sides": (x | lone_o, o, 0, turn),
        "a stone stands on a wall": (x, o, walls | lone_x, turn),
        "a side has no stone": (x, 0, walls, turn),
        "the position is finished": (x, o, full, turn),
        "bits beyond the 49 cells": (x, o, 1 << 49, turn),
        "neither 0 (x) nor 1 (o)": (x, o, walls, 2),
    }
    for words, entry in bad.items():
        msg = _refused(e, lambda: e.set_start_pool([pool[0], entry, pool[1]]), words)
        assert "azh_engine_set_start_pool: entry 1 " in msg
    assert [e.uid_blockers(u) for u in range(4)] == [pool[u % 2][2] for u in range(4)]          # the pool that was set stands
    _refused(e, lambda: e.set_start_pool([pool[0]], stride=0), "stride")
    # random symmetry against an asymmetric entry, both orders, in the engine's existing words
    words = "a blockers mask (0x%x) that is not its own image under all 8 symmetries" % pool[2][2]
    sym = spf.device_engine(pool[0], 4, VISITS)
    sym.set_random_symmetry(True)
    assert "azh_engine_set_start_pool: the random symmetry is not supported with " in _refused(
        sym, lambda: sym.set_start_pool([pool[1], pool[2]]), words)
    sym.set_start_pool([pool[0], pool[1]])                                                  # (two invariant masks: taken)
    other = spf.pooled_engine([pool[1], pool[2]], 4, VISITS)
    assert "azh_engine_set_random_symmetry: not supported with " in _refused(other, lambda: other.set_random_symmetry(True), words)
    # every one of them still plays, and a pool comes too late after the first select
    for eng in (e, sym, other):
        for _ in range(3):
            eh.step(eng)
        _refused(eng, lambda: eng.set_start_pool(pool), "has begun to search")
        _refused(eng, lambda: eng.set_start_pool([]), "has begun to search")
        eh.step(eng)


# ------------------------------------------------------------------ command lines

def _cells_to_packed(cells, turn):
    x = sum(1 << (c % 7 + 7 * (6 - c // 7)) for c, v in enumerate(cells) if v == 1)
    o = sum(1 << (c % 7 + 7 * (6 - c // 7)) for c, v in enumerate(cells) if v == 2)
    return [x | (turn << 63), o]


def test_generator_and_trainer_on_a_three_map_file(tmp_path):
    pool = spf.entries()[1:]                       # three walled maps (the trainer counts the maps of the games with walls)
    maps = tmp_path / "maps.txt"
    maps.write_text("# three maps\n" + "\n".join(spf.fen_of(entry) for entry in pool) + "\n")
    res, path = eh.generator(tmp_path, "--start-fens", str(maps), "--streams", "1")
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    with open(path) as f:
        lines = [json.loads(line) for line in f]
    assert len(lines) == 20
    totals = json.loads(next(l for l in res.stdout.decode().splitlines() if l.startswith("Totals: "))[len("Totals: "):])
    # uid order: the lines are the games 0, 1, 2, ... without the dropped ones (cut at 400 plies), whose number the run reports —
    # line i of a run that drops no game is entry i mod 3
    uid, skipped = 0, 0
    for i, entry in enumerate(lines):
        while entry["blockers"] != link.blockers_to_cells(pool[uid % 3][2]):
            uid, skipped = uid + 1, skipped + 1
            assert skipped <= totals["dropped"], (i, uid, totals["dropped"])
        x, o, walls, turn = pool[uid % 3]
        uid += 1
        boards = np.array([_cells_to_packed(b, (turn + p) % 2) for p, b in enumerate(entry["boards"])], dtype=np.uint64)
        assert boards[0].tolist() == [x | (turn << 63), o]
        stones = (boards[:, 0] & np.uint64((1 << 63) - 1)) | boards[:, 1]
        assert not (stones & np.uint64(walls)).any(), i                              # no stone ever stands on a wall
        moves, counts, results = link.rules_batch(boards, walls)
        for p, text in enumerate(entry["moves"]):
            assert results[p] == 0 and orc.move_from_string(text) in moves[p, :counts[p]].tolist(), (i, p, text)
    assert skipped == totals["dropped"] and {json.dumps(e["blockers"]) for e in lines} == {
        json.dumps(link.blockers_to_cells(entry[2])) for entry in pool}
    new = str(tmp_path / "model-005.npy")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--steps", "2", "--minibatch-size", "16", "--games", path,
                          "--old-path", str(tmp_path / "model-004.npy"), "--new-path", new, "--device-samples"],
                         cwd=ROOT, capture_output=True, timeout=300)
    assert out.returncode == 0 and os.path.exists(new), out.stderr.decode()[-3000:]
    assert "; 20 games on 3 wall maps." in out.stdout.decode()


def test_match_with_two_maps_plays_each_pairing_on_one_map():
    pool = [spf.entries()[2], spf.entries()[1]]
    weights = [model.random_init(1, 128, seed=s) for s in (5, 6)]
    match = arena.Match(weights[0], weights[1], 6, games=8, dtype="f16", seed=11, start_fens=[spf.fen_of(e) for e in pool])
    match.set_game_limit(8)
    games = {}
    for _ in range(200):
        match.run(50)
        for g in match.drain():
            games[g["uid"]] = g
        if len(games) == 8:
            break
    assert sorted(games) == list(range(8))
    for k in range(4):
        x, o, walls, turn = pool[k % 2]
        first = [v for v in _start_cells(x, o)]
        for uid in (2 * k, 2 * k + 1):
            assert games[uid]["boards"][0] == first, uid                   # both games of pairing k start from map k mod 2
            assert games[uid]["white"] == ("a" if uid % 2 == 0 else "b")
            for b in games[uid]["boards"]:
                assert all(b[c] == 0 for c in link.blockers_to_cells(walls)), uid
    match.close()


def _start_cells(x, o):
    return [1 if (x >> (c % 7 + 7 * (6 - c // 7))) & 1 else 2 if (o >> (c % 7 + 7 * (6 - c // 7))) & 1 else 0 for c in range(49)]


def test_records_of_a_pooled_engine_enter_the_store_with_their_own_masks(tmp_path):
    """(in a process of its own: the sample store wants torch's HIP runtime loaded before the library, tests/samples_gpu_checks.py)"""
    verdicts = fresh_process.verdicts_of("tests.start_pool_store_check", str(tmp_path / "verdicts.json"), timeout=300)
    fresh_process.passed(verdicts, "check_records_enter_the_store_with_their_own_masks")
