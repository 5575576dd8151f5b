"""The recorded search value and resignation (azh_engine_set_resign), the parts that need no device: the "values" and
"resigned" keys of a game line, the play-through draw against a restatement on the oracle's Philox, the numpy restatement of
the rule on hand-made sequences, the trainer's value blend and the calibration tool."""
import ctypes
import json
import math
import os
import random

import numpy as np
import pytest

from ataxxzero_amd import link, training
from oracle import oracle_lib as orc
from tests import resign_reference as ref
from tests.helpers import GOLDEN
from tests.record_fixtures import MAGIC, dumped, random_record, shortest
from tools import resign_calibration

STREAM_RESIGN = 6
SEED = 0x1234567_89ABCDEF


def _bits(q):
    return int(np.array([q], dtype=np.float32).view(np.uint32)[0])


def _valued(rec, qs, fulls=None, resigned=False):
    """the record with kind bit 16 (and 32, and 4 where `fulls` is given) and word 5 of every ply set from qs / fulls"""
    rec = rec.copy()
    rec[7] |= 16 | (32 if resigned else 0) | (4 if fulls is not None else 0)
    pos = 8
    for p, q in enumerate(qs):
        rec[pos + 5] = (_bits(q) & 0x7FFFFFFF) | ((0x80000000 if fulls[p] else 0) if fulls is not None else 0)
        pos += 6 + (int(rec[pos + 4]) >> 16)
    assert pos == rec[5]
    return rec


def test_values_and_resigned_keys_of_a_game_line():
    rng = np.random.default_rng(11)
    for case in range(16):
        plies = int(rng.integers(1, 25))
        result = 1 + case % 2
        rec, entry = random_record(rng, plies=plies, visits_hi=400, result=result)
        plain = link.format_record_json(rec)
        assert shortest(plain) == dumped(entry) and b"values" not in plain and b"resigned" not in plain
        qs = (rng.integers(0, 401, size=plies).astype(np.float32) / np.float32(rng.integers(1, 401))).clip(0, 1)
        qs = qs.astype(np.float32)
        qs[rng.integers(0, plies)] = np.float32(0.5)
        want = [2 * float(np.float32(q)) - 1 for q in qs]
        fulls = [int(v) for v in rng.integers(0, 2, size=plies)]
        for capped in (False, True):
            for resigned in (False, True):
                line = link.format_record_json(_valued(rec, qs, fulls if capped else None, resigned))
                got = json.loads(line)
                keys = ["boards", "dists"] + ["full"] * capped + ["moves"] + ["resigned"] * resigned + ["result", "values"]
                assert list(got.keys()) == keys
                assert got["values"] == want            # exactly: 2 (double) q - 1
                assert all(-1.0 <= v <= 1.0 for v in got["values"])
                if capped:
                    assert got["full"] == fulls     # the sign bit
                if resigned:
                    assert got["resigned"] == 3 - result
                assert got["result"] == result
                extra = dict(values=want)
                if capped:
                    extra["full"] = fulls
                if resigned:
                    extra["resigned"] = 3 - result
                assert shortest(line) == dumped(dict(entry, **extra))
                ids = json.loads(link.format_record_json(_valued(rec, qs, fulls if capped else None, resigned), with_ids=True))
                assert list(ids.keys()) == keys[:-1] + ["slot", "uid", "values"]
                # the same record with the new bits and word 5 cleared is the line of today, byte for byte
                back = _valued(rec, qs, fulls if capped else None, resigned)
                back[7] &= ~np.uint32(48)
                pos = 8
                for p in range(plies):
                    back[pos + 5] = (fulls[p] if capped else 0)
                    pos += 6 + (int(back[pos + 4]) >> 16)
                old = link.format_record_json(back)
                assert b"values" not in old and b"resigned" not in old
                if capped:
                    assert shortest(old) == dumped(dict(entry, full=fulls))
                else:
                    assert old == plain


def test_a_value_that_is_not_finite_is_written_as_zero():
    rng = np.random.default_rng(5)
    rec, _ = random_record(rng, plies=5, visits_hi=50)
    qs = np.array([np.nan, np.inf, 0.25, 1.0, 0.0], dtype=np.float32)
    line = link.format_record_json(_valued(rec, qs, [1, 0, 1, 0, 1]))
    got = json.loads(line)
    assert got["values"] == [0.0, 0.0, -0.5, 1.0, -1.0] and got["full"] == [1, 0, 1, 0, 1]
    assert b"null" not in line and b"nan" not in line.lower()


def test_unknown_kind_bits_are_still_rejected():
    rng = np.random.default_rng(6)
    rec, _ = random_record(rng, plies=3, visits_hi=9)
    for kind in (16, 32, 48, 16 | 4, 16 | 8, 2 | 16 | 32, 60 | 2):
        ok = rec.copy()
        ok[7] = kind
        link.format_record_json(ok)
    for kind in (64, 128, 16 | 64, 3 | 16, 1 | 16, 1 << 31):
        bad = rec.copy()
        bad[7] = kind
        with pytest.raises(link.AzhError):
            link.format_record_json(bad)
    marker = np.array([MAGIC, 0, 0, 0, 0, 8, 0, 17], dtype=np.uint32)
    with pytest.raises(link.AzhError):
        link.format_record_json(marker)


def restated_playthrough(seed, uid, per_65536):
    """play-through iff (philox(k0, k1, uid, 0, STREAM_RESIGN, 0).v[0] >> 16) < per_65536"""
    out = (ctypes.c_uint32 * 4)()
    orc.lib().orc_probe_philox(seed, uid, 0, STREAM_RESIGN, 0, out)
    return int((out[0] >> 16) < per_65536)


def test_playthrough_equals_the_restatement_on_the_oracles_philox():
    rng = np.random.default_rng(1)
    uids = list(range(64)) + [4095, 4096, 0xFFFFFFFF] + [int(v) for v in rng.integers(0, 1 << 32, size=1981)]
    seeds = [SEED, SEED ^ (1 << 40)]
    pairs = [(s, u) for s in seeds for u in uids]
    assert len(pairs) == 4096
    for share in (0, 1, 16384, 65536):
        got = [link.resign_playthrough(s, u, share) for s, u in pairs]
        assert got == [restated_playthrough(s, u, share) for s, u in pairs], share
        if share == 0:
            assert not any(got)
        if share == 65536:
            assert all(got)
    n = len(uids)
    a = [link.resign_playthrough(seeds[0], u, 16384) for u in uids]
    b = [link.resign_playthrough(seeds[1], u, 16384) for u in uids]
    assert a != b                                       # the high half of the seed is part of the key
    sd = (n * 0.25 * 0.75) ** 0.5
    assert abs(sum(a) - 0.25 * n) <= 5 * sd
    # the draw is not the playout cap's at ply 0 (stream 4) nor the symmetry key's (stream 5)
    assert a != [link.playout_cap_kind(seeds[0], u, 0, 16384) for u in uids]


def _plies(rows):
    return [(m, ref.q_bits(np.float32(q)), c) for m, q, c in rows]


def test_reference_rule_on_hand_made_sequences():
    T = 0.2
    lo, hi = 0.1, 0.6
    # counters per side: x is below at its plies 0, 2; o is fine
    seq = _plies([(1, lo, True), (2, hi, True), (1, lo, True), (2, hi, True)])
    assert ref.replay(seq, T, 2) == [False, False, True, False] and ref.first_fire(seq, T, 2) == (2, 1)
    assert ref.replay(seq, T, 1) == [True, False, True, False]
    assert ref.first_fire(seq, T, 3) is None
    # the other side's bad plies do not add to mine: x, o, x, o each once below in turn
    seq = _plies([(1, lo, True), (2, lo, True), (1, hi, True), (2, hi, True), (1, lo, True), (2, lo, True)])
    assert ref.replay(seq, T, 2) == [False] * 6
    # o alone fires
    seq = _plies([(1, hi, True), (2, lo, True), (1, hi, True), (2, lo, True)])
    assert ref.first_fire(seq, T, 2) == (3, 2)
    # reset on a good ply
    seq = _plies([(1, lo, True), (2, hi, True), (1, hi, True), (2, hi, True), (1, lo, True), (2, hi, True), (1, lo, True)])
    assert ref.replay(seq, T, 2) == [False] * 6 + [True]
    # a ply equal to the threshold is not below
    seq = _plies([(1, lo, True), (2, hi, True), (1, np.float32(T), True), (2, hi, True), (1, lo, True)])
    assert ref.replay(seq, T, 2) == [False] * 5
    # FAST plies are skipped: they neither advance ...
    seq = _plies([(1, lo, True), (2, hi, True), (1, lo, False), (2, hi, True), (1, hi, True), (2, hi, True), (1, lo, True)])
    assert ref.replay(seq, T, 2) == [False] * 7
    # ... nor reset
    seq = _plies([(1, lo, True), (2, hi, True), (1, hi, False), (2, hi, True), (1, lo, True)])
    assert ref.replay(seq, T, 2) == [False, False, False, False, True]
    # NaN is never below, and resets
    seq = _plies([(1, lo, True), (2, hi, True), (1, np.nan, True), (2, hi, True), (1, lo, True), (2, np.nan, True),
                  (1, lo, True)])
    assert ref.replay(seq, T, 2) == [False] * 6 + [True]
    seq = _plies([(1, np.nan, True), (2, np.nan, True)] * 4)
    assert ref.replay(seq, T, 1) == [False] * 8
    # q_below = 0 never fires (q is never negative; -0.0 and 0.0 are not below 0)
    seq = _plies([(1, 0.0, True), (2, 0.0, True)] * 5)
    assert ref.replay(seq, 0.0, 1) == [False] * 10
    # a play-through game goes on counting: the rule fires at every later bad ply too; counters stop at 255
    seq = _plies([(1, lo, True), (2, hi, True)] * 300)
    fired = ref.replay(seq, T, 255)
    assert fired.index(True) == 2 * 254 and all(fired[2 * 254::2]) and not any(fired[1::2])
    # consecutive = 0 is off
    assert ref.replay(seq[:6], T, 0) == [False] * 6


def test_reference_value_of_a_root():
    q, ok = ref.ply_value([3, 7, 7, 1], np.array([1.5, 2.0, 6.0, 1.0], dtype=np.float32))
    assert ok and q == np.float32(2.0) / np.float32(7.0)             # the tie goes to the lowest index
    q, ok = ref.ply_value([0, 0], [0.0, 0.0])
    assert not ok and q == np.float32(0.5)
    q, ok = ref.ply_value([], [])
    assert not ok and q == np.float32(0.5)
    q, ok = ref.ply_value([1, 4], np.array([1.0, np.nan], dtype=np.float32))
    assert ok and math.isnan(float(q))
    assert ref.decode_word5(0x80000000 | ref.q_bits(np.float32(0.25)), True) == (ref.q_bits(np.float32(0.25)), True)
    assert ref.decode_word5(ref.q_bits(np.float32(0.25)), True) == (ref.q_bits(np.float32(0.25)), False)
    assert ref.decode_word5(ref.q_bits(np.float32(0.25)), False) == (ref.q_bits(np.float32(0.25)), True)


def _entries():
    with open(os.path.join(GOLDEN, "train_entries.json")) as f:
        return json.load(f)


def test_value_blend_of_the_trainer():
    base = _entries()
    rng = np.random.default_rng(3)
    valued = []
    for e in base[:4]:
        e = dict(e)
        e.pop("random_ply", None)
        e["values"] = [2 * float(np.float32(v)) - 1 for v in rng.random(len(e["boards"]))]
        valued.append(e)
    entries = valued + base[4:]          # entries with and without "values"
    assert any("values" not in e for e in entries)
    for L in (0.25, 0.5, 1.0):
        blended = 0
        for seed in range(3):
            random.seed(seed)
            a = training.make_minibatch_reference(entries, 100, value_blend=L)
            state = random.getstate()
            random.seed(seed)
            b = training.make_minibatch(entries, 100, value_blend=L)
            assert random.getstate() == state
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and np.array_equal(x, y)
            random.seed(seed)
            z = training.make_minibatch(entries, 100)
            assert np.array_equal(z[0], b[0]) and np.array_equal(z[1], b[1])      # the same draws
            assert set(np.unique(z[2])) <= {-1.0, 1.0}
            blended += int((z[2] != b[2]).sum())
            assert (np.abs(b[2]) <= 1).all()
        assert blended > 50
    # one sample by hand
    e = valued[0]
    random.seed(2)
    f, p, v = training.get_sample_from_entries([e], value_blend=0.25)
    random.seed(2)
    f0, p0, v0 = training.get_sample_from_entries([e])
    assert np.array_equal(f, f0) and np.array_equal(p, p0) and v0[0] in (1, -1)
    shown = [i for i in range(len(e["boards"])) for sym in range(8) if np.array_equal(
        f, training.apply_symmetry(sym, training.board_to_features(e["boards"][i], 1 + i % 2)))]
    assert shown and any(v[0] == 0.75 * v0[0] + 0.25 * e["values"][i] for i in shown)
    assert v[0] != v0[0]
    # L = 0 is the call without the argument, bit for bit, on entries with values too
    for seed in range(3):
        random.seed(seed)
        a = training.make_minibatch(entries, 100)
        sa = random.getstate()
        random.seed(seed)
        b = training.make_minibatch(entries, 100, value_blend=0.0)
        assert random.getstate() == sa
        random.seed(seed)
        c = training.make_minibatch_reference(entries, 100, 0.0)
        for x, y, w in zip(a, b, c):
            assert x.tobytes() == y.tobytes() == w.tobytes()


def _game(values, result, full=None, resigned=None):
    e = {"boards": [[0] * 49] * len(values), "moves": ["a1"] * len(values), "result": result, "values": values}
    if full is not None:
        e["full"] = full
    if resigned is not None:
        e["resigned"] = resigned
    return e


def test_calibration_tool_counts(tmp_path, capsys):
    # g0: x below -0.8 at plies 2, 4 (x loses: a true positive at K = 2, ply 4; 3 plies saved of 8)
    g0 = _game([0.0, 0.1, -0.9, 0.2, -0.95, 0.3, -1.0, 0.5], 2)
    # g1: o below at plies 1, 3, but o WINS (a false positive at ply 3; 2 plies saved of 6)
    g1 = _game([0.5, -0.9, 0.5, -0.85, 0.5, 0.9], 2)
    # g2: never two in a row: x below at 0, fine at 2, below at 4
    g2 = _game([-0.9, 0.0, 0.1, 0.0, -0.9, 0.0], 1)
    # g3: with the playout cap: x below at ply 0 (full), ply 2 is FAST and skipped, ply 4 (full) below -> fires at 4
    g3 = _game([-0.9, 0.0, 0.9, 0.0, -0.9, 0.0, 0.0], 2, full=[1, 1, 0, 1, 1, 1, 1])
    # g4: a resigned game is not used; g5: a line without values is not used
    g4 = _game([-0.9, 0.0, -0.9], 2, resigned=1)
    g5 = {"boards": [[0] * 49], "moves": ["a1"], "result": 1}
    entries = [g0, g1, g2, g3, g4, g5]
    assert resign_calibration.would_resign(g0, -0.8, 2) == 4
    assert resign_calibration.would_resign(g0, -0.8, 3) == 6
    assert resign_calibration.would_resign(g0, -0.8, 1) == 2
    assert resign_calibration.would_resign(g1, -0.8, 2) == 3
    assert resign_calibration.would_resign(g1, -0.9, 2) is None          # -0.9 is not below -0.9
    assert resign_calibration.would_resign(g2, -0.8, 2) is None
    assert resign_calibration.would_resign(g3, -0.8, 2) == 4
    n, total, rows = resign_calibration.calibrate(entries, [-0.8, -0.99], [1, 2])
    assert (n, total) == (4, 8 + 6 + 6 + 7)
    by = {(v, k): (ended, wrong, saved) for v, k, ended, wrong, saved in rows}
    assert by[(-0.8, 2)] == (3, 1, 3 + 2 + 2)
    # K = 1: g0 at ply 2 (5 saved), g1 at ply 1 (4 saved, o wins: wrong), g2 at ply 0 (5 saved; x wins: wrong), g3 at ply 0 (6)
    assert by[(-0.8, 1)] == (4, 2, 5 + 4 + 5 + 6)
    # below -0.99: only g0's last ply, -1.0 (x loses; one ply saved)
    assert by[(-0.99, 1)] == (1, 0, 1) and by[(-0.99, 2)] == (0, 0, 0)
    path = tmp_path / "games.json"
    path.write_text("".join(json.dumps(e) + "\n" for e in entries))
    assert resign_calibration.main([str(path), "--thresholds", "-0.8", "--plies", "2"]) == 0
    out = capsys.readouterr().out
    assert "6 lines, 4 of them with values and not resigned, 27 plies" in out
    row = out.strip().splitlines()[-1].split()
    assert row[:4] == ["-0.800", "2", "3", "75.0%"] and row[4:6] == ["1", "33.3%"] and row[6] == "25.9%"
