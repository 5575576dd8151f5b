"""The device-resident sample store (azh_samples_*), the parts that need no device: ring records packed into the store's
arrays against the parse of the same games' own lines, malformed records, entries converted for the store against
training._entry_arrays, and the device's draw restated on the oracle's Philox."""
import ctypes
import json

import numpy as np
import pytest

from ataxxzero_amd import link, training
from tests import aux_fixtures as afx
from tests import walls_fixtures as wf
from tests.samples_fixtures import (BAD, FULL, HAS_FULL, HAS_VALUES, PASS, _arrays_equal, draw_mirror, marker,
                                    random_record, restated_draw)

SEED = 0x1234567_89ABCDEF


def record_cases():
    rng = np.random.default_rng(2024)
    recs = []
    for case in range(48):
        kind = [0, 4, 16, 4 | 16, 16 | 32, 4 | 8, 4 | 8 | 16 | 32, 8][case % 8]
        plies = 1 if case == 5 else int(rng.integers(2, 30))
        recs.append(random_record(
            rng, plies, [1, 7, 400, 2000, 60000, 65535][case % 6], kind=kind,
            random_ply=int(rng.integers(0, plies - 1)) if case % 4 == 3 and plies > 1 else None, result=1 + case % 2,
            zero_total_at=0 if case % 10 == 9 else None, empty_at=plies - 1 if case % 7 == 6 else None, uid=case))
        if case % 5 == 2:
            recs.append(marker(1000 + case))         # a dropped game's marker in between
    return recs


def test_packed_records_equal_the_parse_of_their_own_lines():
    recs = record_cases()
    packed = link.pack_records(np.concatenate(recs))
    games = [r for r in recs if r[7] != 1]
    entries = [json.loads(link.format_record_json(r)) for r in games]
    assert len(packed.games) == len(games) == 48
    kinds = {int(r[7]) for r in games}
    assert {0, 4, 16, 20, 48, 12, 60, 8} <= kinds
    _arrays_equal(packed, link.entries_to_arrays(entries))
    # and against training._entry_arrays and the lines themselves, array by array
    ply = target = 0
    for g, (rec, entry) in enumerate(zip(games, entries)):
        cells, idx, wts, start = training._entry_arrays(entry)
        n = len(entry["boards"])
        first, plies, word, random_ply_1 = (int(v) for v in packed.games[g])
        assert (first, plies, word & 0xFF) == (ply, n, entry["result"])
        assert random_ply_1 == entry.get("random_ply", -1) + 1
        assert bool(word & HAS_FULL) == ("full" in entry) == bool(rec[link.REC_KIND] & link.REC_KIND_PLAYOUT_CAP)
        assert bool(word & HAS_VALUES) == ("values" in entry) == bool(rec[link.REC_KIND] & link.REC_KIND_VALUES)
        for p in range(n):
            x, o = (int(v) for v in packed.boards[ply + p])
            want = [1 if x >> (c % 7 + 7 * (6 - c // 7)) & 1 else 2 if o >> (c % 7 + 7 * (6 - c // 7)) & 1 else 0
                    for c in range(49)]
            assert want == entry["boards"][p] and not x & o
            assert int(packed.ply_flags[ply + p]) == (FULL if entry.get("full", [0] * n)[p] else 0)
            assert packed.values[ply + p].tobytes() == np.float64(entry.get("values", [0.0] * n)[p]).tobytes()
            lo, hi = (int(v) for v in packed.target_start[ply + p:ply + p + 2])
            assert (lo - target, hi - target) == (int(start[p]), int(start[p + 1]))
            assert list(packed.target_index[lo:hi]) == list(idx[start[p]:start[p + 1]])
            assert packed.target_weight[lo:hi].tobytes() == wts[start[p]:start[p + 1]].tobytes()
        ply += n
        target += int(start[-1])
    assert (ply, target) == (len(packed.ply_flags), len(packed.target_index))
    values = packed.values[packed.values != 0]
    assert len(values) and np.isfinite(packed.values).all()       # q = nan / inf read 0
    assert (packed.target_weight == 0).any()                      # the zero-total plies


def test_malformed_records_are_refused_and_add_nothing():
    rng = np.random.default_rng(7)
    good = [random_record(rng, 6, 50, uid=u) for u in range(3)]
    whole = np.concatenate(good)
    n_games = len(link.pack_records(whole).games)
    assert n_games == 3

    def refused(words):
        outs = [np.full(4096, 0xAB, dtype=np.uint8) for _ in range(7)]
        arrays = link.CSampleArrays(99, 9999, 99999, *[o.ctypes.data for o in outs])
        rc = link.load().azh_samples_pack_records(words.ctypes.data, words.size, 0, None, 0, 0, ctypes.byref(arrays))
        assert rc == -2, rc
        assert (arrays.n_games, arrays.n_plies, arrays.n_targets) == (99, 9999, 99999)
        assert all((o == 0xAB).all() for o in outs)                                    # nothing written
        with pytest.raises(link.AzhError):
            link.pack_records(words)

    refused(np.ascontiguousarray(whole[:-1]))                     # the last record is cut short
    wrong = whole.copy()
    wrong[len(good[0]) + 5] += 1                                  # the second record's word count is off by one
    refused(wrong)
    long = whole.copy()
    long[len(good[0]) + 8 + 4] += 200 << 16                       # nd of its first ply runs past its end
    refused(long)
    more = whole.copy()
    more[3] += 1                                                  # one ply more than the words hold
    refused(more)
    no_move = whole.copy()
    no_move[8 + 6] = (no_move[8 + 6] & 0xFFFF0000) | (0 | 1 << 8)  # a1 -> b1: neither a clone nor a jump
    refused(no_move)
    junk = np.concatenate([good[0], np.array([5], dtype=np.uint32), good[1]])
    refused(junk)                                                 # a stray word between two records


def walled_records():
    """A game on the default walls, a dropped game's marker, a game on the asymmetric walls -> (records, a mask for each)."""
    recs, masks = [], []
    for uid, fen in ((0, wf.DEFAULT_FEN), (2, wf.ASYMMETRIC_FEN)):
        entry, positions = afx.passless_games(fen, 1)[0]
        recs.append(afx.record_of(entry, positions, uid))
        masks.append(positions[0].masks()[2])
    assert masks[0] and masks[1] and masks[0] != masks[1]
    return [recs[0], marker(1), recs[1]], [masks[0], masks[0], masks[1]]


def test_two_ways_to_give_walls_are_refused_together_and_a_wrong_mask_count_writes_nothing():
    recs, masks = walled_records()
    words = np.concatenate(recs)
    pack = link.load().azh_samples_pack_records
    for aux in (0, 1):
        for n_masks, blockers, want in ((3, masks[0], -1), (2, 0, -2), (4, 0, -2)):
            given = np.array(masks + [0], dtype=np.uint64)
            outs = [np.full(1 << 16, 0xAB, dtype=np.uint8) for _ in range(9)]
            arrays = link.CSampleArrays(99, 9999, 99999, *[o.ctypes.data for o in outs])
            rc = pack(words.ctypes.data, words.size, blockers, given.ctypes.data, n_masks, aux, ctypes.byref(arrays))
            assert rc == want, (aux, n_masks, rc)
            assert (arrays.n_games, arrays.n_plies, arrays.n_targets) == (99, 9999, 99999)
            assert all((o == 0xAB).all() for o in outs)
    with pytest.raises(link.AzhError, match="error -2"):
        link.pack_records(words, np.array(masks[:2], dtype=np.uint64))
    assert len(link.pack_records(words, np.array(masks, dtype=np.uint64)).games) == 2


@pytest.mark.parametrize("aux", [False, True])
def test_packing_with_a_mask_per_record_is_packing_each_record_with_its_own(aux):
    recs, masks = walled_records()
    whole = link.pack_records(np.concatenate(recs), np.array(masks, dtype=np.uint64), aux=aux)
    first, second = (link.pack_records(recs[k], masks[k], aux=aux) for k in (0, 2))
    assert len(link.pack_records(recs[1], masks[1], aux=aux).games) == 0          # the marker alone: no game
    plies, targets = len(first.ply_flags), len(first.target_index)
    moved = second.games.copy()
    moved[:, 0] += plies
    want = {"games": np.concatenate([first.games, moved]),
            "target_start": np.concatenate([first.target_start, second.target_start[1:] + targets]).astype(np.int32)}
    if not aux:
        assert whole.owners is None and first.owners is None and second.owners is None
    for name in link.SampleArrays.__slots__ + (("owners",) if aux else ()):
        got = getattr(whole, name)
        expect = want.get(name)
        if expect is None:
            expect = np.concatenate([getattr(first, name), getattr(second, name)])
        assert got.dtype == expect.dtype and got.shape == expect.shape, name
        assert got.tobytes() == expect.tobytes(), name
    assert whole.blockers.tolist() == [masks[0], masks[2]]
    assert len(whole.games) == 2 and (plies, targets) != (0, 0) and (not aux or whole.owners.any())


def test_entries_for_the_store_follow_entry_arrays():
    """pass plies and "pass" keys, list-typed moves, an entry without dists, "full", "values", random_ply."""
    board = [0] * 49
    entries = [
        {"boards": [board] * 3, "moves": ["a1", "pass", "a1c3"], "result": 2,
         "dists": [{"a1": 0.25, "pass": 0.5, "b2": 0.25}, {}, {"a1c3": 1.0}], "full": [1, 0, 1], "values": [0.5, -1.0, 0.125]},
        {"boards": [[1] * 49, [2] * 49], "moves": [["c", [3, 4]], [[0, 0], [2, 1]]], "result": 1, "random_ply": 0},
    ]
    a = link.entries_to_arrays(entries)
    assert a.games.tolist() == [[0, 3, 2 | HAS_FULL | HAS_VALUES, 0], [3, 2, 1, 1]]
    assert a.ply_flags.tolist() == [FULL, PASS, FULL, 0, 0]
    assert a.values.tolist() == [0.5, -1.0, 0.125, 0.0, 0.0]
    assert a.target_start.tolist() == [0, 2, 2, 3, 4, 5]
    want = [training._flat_policy_index(m) for m in ("a1", "b2", "a1c3", ["c", [3, 4]], [[0, 0], [2, 1]])]
    assert a.target_index.tolist() == want
    assert a.target_weight.tolist() == [0.25, 0.25, 1.0, 1.0, 1.0]
    assert a.boards.tolist() == [[0, 0]] * 3 + [[(1 << 49) - 1, 0], [0, (1 << 49) - 1]]


# ---------------------------------------------------------------- the draw


def test_draw_equals_the_restatement_on_the_oracles_philox():
    games, flags, can = draw_mirror()
    most = 0
    seen = set()
    for step in range(3):
        for i in range(257):
            got = link.samples_draw(SEED, step, i, 0, 40, games, flags)
            assert got == restated_draw(SEED, step, i, 0, 40, games, flags), (step, i)
            g, ply, sym, attempts = got
            assert 1 <= attempts <= 64 and g >= 0                  # half the games undrawable: 64 misses have chance 2^-64
            assert can[g] and 0 <= sym < 8 and ply < games[g][1]
            assert not flags[games[g][0] + ply] & (PASS | BAD)
            if games[g][3]:
                assert ply == games[g][3]
            elif games[g][2] & HAS_FULL:
                assert flags[games[g][0] + ply] & FULL
            most = max(most, attempts)
            seen.add(g)
    assert most > 3 and seen == {g for g in range(40) if can[g]}
    # a sub-range, and another key
    for i in range(64):
        got = link.samples_draw(SEED ^ 1 << 40, 7, i, 10, 30, games, flags)
        assert got == restated_draw(SEED ^ 1 << 40, 7, i, 10, 30, games, flags) and 10 <= got[0] < 40


def test_a_range_of_undrawable_games_exhausts_the_attempts():
    games, flags, can = draw_mirror()
    g = can.index(False)
    assert link.samples_draw(SEED, 0, 0, g, 1, games, flags) == (-1, -1, -1, 64)
    with pytest.raises(link.AzhError):
        link.samples_draw(SEED, 0, 0, 30, 11, games, flags)       # past the last game
