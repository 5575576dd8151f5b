"""Playout cap randomization, the parts that need no device: the kind of a ply as a pure function of (seed, uid, ply)
against a restatement on the oracle's Philox, the "full" key of a game line, and the training sampler that draws its
policy targets from the FULL plies only."""
import ctypes
import json
import os
import random

import numpy as np

from ataxxzero_amd import link, training
from oracle import oracle_lib as orc
from tests.helpers import GOLDEN
from tests.record_fixtures import MAGIC, dumped, random_record, shortest

STREAM_PLAYOUT_CAP = 4
SEED = 0x1234567_89ABCDEF


def restated_kind(seed, uid, ply, full_per_65536):
    """FULL iff (philox(k0, k1, uid, ply, STREAM_PLAYOUT_CAP, 0).v[0] >> 16) < full_per_65536"""
    out = (ctypes.c_uint32 * 4)()
    orc.lib().orc_probe_philox(seed, uid, ply, STREAM_PLAYOUT_CAP, 0, out)
    return int((out[0] >> 16) < full_per_65536)


def test_kind_equals_the_restatement_on_the_oracles_philox():
    rng = np.random.default_rng(1)
    uids = [0, 1, 4095, 0xFFFFFFFF] + [int(v) for v in rng.integers(0, 1 << 32, size=60)]
    plies = list(range(60)) + [399, 400, 65535, 0xFFFFFFFF]
    pairs = [(u, p) for u in uids for p in plies]
    assert len(pairs) == 4096
    for frac in (0, 1, 16384, 65536):
        got = [link.playout_cap_kind(SEED, u, p, frac) for u, p in pairs]
        assert got == [restated_kind(SEED, u, p, frac) for u, p in pairs], frac
        if frac == 0:
            assert not any(got)
        if frac == 65536:
            assert all(got)
    # the high half of the seed is part of the key
    a = [link.playout_cap_kind(SEED, u, p, 32768) for u, p in pairs]
    b = [link.playout_cap_kind(SEED ^ (1 << 40), u, p, 32768) for u, p in pairs]
    assert a != b


def test_a_quarter_of_the_plies_is_full_at_16384():
    n = 65536
    full = sum(link.playout_cap_kind(20260101, uid, ply, 16384) for uid in range(256) for ply in range(256))
    sd = (n * 0.25 * 0.75) ** 0.5
    assert abs(full - 0.25 * n) <= 5 * sd, (full, 0.25 * n, sd)


def _capped(rec, kinds):
    """the record with the header's playout-cap flag and word 5 of every ply set from `kinds`"""
    rec = rec.copy()
    rec[7] |= 4
    pos = 8
    for k in kinds:
        rec[pos + 5] = k
        pos += 6 + (int(rec[pos + 4]) >> 16)
    assert pos == rec[5]
    return rec


def test_full_key_is_written_in_its_sorted_place_only_with_the_header_flag():
    rng = np.random.default_rng(3)
    for case in range(12):
        plies = int(rng.integers(1, 25))
        rec, entry = random_record(rng, plies=plies, visits_hi=400, result=1 + case % 2)
        plain = link.format_record_json(rec)
        assert shortest(plain) == dumped(entry) and b"full" not in plain
        kinds = [int(v) for v in rng.integers(0, 2, size=plies)]
        line = link.format_record_json(_capped(rec, kinds))
        got = json.loads(line)
        assert list(got.keys()) == ["boards", "dists", "full", "moves", "result"]
        assert got["full"] == kinds
        assert shortest(line) == dumped(dict(entry, full=kinds))
        # without the "full" key the capped line is the plain line, byte for byte
        key = b',"full":[' + b",".join(str(k).encode() for k in kinds) + b"]"
        assert line.replace(key, b"") == plain
        ids = link.format_record_json(_capped(rec, kinds), with_ids=True)
        assert list(json.loads(ids).keys()) == ["boards", "dists", "full", "moves", "result", "slot", "uid"]
        # ply words set but no header flag (a game of an engine with the mode off never has them): the existing bytes
        noflag = _capped(rec, kinds)
        noflag[7] &= ~np.uint32(4)
        assert link.format_record_json(noflag) == plain
    # a partial game (kind 2) with the flag is still a record; a dropped-game marker with it is not
    rec, _ = random_record(rng, plies=3, visits_hi=9)
    part = _capped(rec, [1, 0, 1])
    part[7] |= 2
    assert json.loads(link.format_record_json(part))["full"] == [1, 0, 1]
    bad = np.array([MAGIC, 0, 0, 0, 0, 8, 0, 5], dtype=np.uint32)
    try:
        link.format_record_json(bad)
    except link.AzhError:
        pass
    else:
        raise AssertionError("a marker with the cap flag was formatted")


def _entries():
    with open(os.path.join(GOLDEN, "train_entries.json")) as f:
        return json.load(f)


def _with_full(entry, full):
    e = dict(entry)
    e.pop("random_ply", None)
    e["full"] = list(full)
    return e


def test_sampler_draws_from_full_plies_only_and_skips_entries_without_one():
    base = _entries()     # dists / one-hot / random_ply flavours (the latter's key is dropped: the cap refuses that mode)
    assert len(base) == 6 and not any("pass" in e["moves"] for e in base)
    rng = np.random.default_rng(7)
    capped = [_with_full(e, (rng.random(len(e["boards"])) < 0.25).astype(int).tolist()) for e in base[:4]]
    assert all(any(e["full"]) and not all(e["full"]) for e in capped)
    none_full = _with_full(base[4], [0] * len(base[4]["boards"]))
    entries = capped + [none_full]

    def full_boards(e):
        """feature planes of the FULL plies of e, under all 8 symmetries"""
        return {training.apply_symmetry(s, training.board_to_features(e["boards"][p], 1 + p % 2)).tobytes()
                for p, f in enumerate(e["full"]) if f for s in range(8)}

    allowed = set().union(*[full_boards(e) for e in capped])
    fast = set()
    for e in entries:
        for p, f in enumerate(e["full"]):
            if not f:
                fast |= {training.apply_symmetry(s, training.board_to_features(e["boards"][p], 1 + p % 2)).tobytes()
                         for s in range(8)}
    fast -= allowed   # (a position may recur at a full ply)
    random.seed(11)
    seen = set()
    for _ in range(400):
        f, p, v = training.get_sample_from_entries(entries)
        key = np.asarray(f).tobytes()
        assert key in allowed and key not in fast
        assert abs(p.sum() - 1) < 1e-3
        seen.add(key)
    assert len(seen) > 20
    # the batched pipeline: the same draws, the same arrays
    for seed in range(3):
        random.seed(seed)
        a = training.make_minibatch_reference(entries, 100)
        state = random.getstate()
        random.seed(seed)
        b = training.make_minibatch(entries, 100)
        assert random.getstate() == state
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert all(row.tobytes() in allowed for row in a[0].astype(np.int8))
    # an entry all of whose plies are full samples exactly like the same entry without the key
    every = [_with_full(e, [1] * len(e["boards"])) for e in base]
    plain = [{k: v for k, v in e.items() if k != "full"} for e in every]
    random.seed(5)
    a = training.make_minibatch_reference(every, 50)
    random.seed(5)
    b = training.make_minibatch_reference(plain, 50)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_entries_without_the_key_sample_as_before():
    entries = _entries()
    assert not any("full" in e for e in entries)
    want = np.load(os.path.join(GOLDEN, "train_samples.npz"))
    for seed in range(64):
        random.seed(seed)
        f, p, v = training.get_sample_from_entries(entries)
        assert (np.asarray(f) == want["features"][seed]).all(), seed
        assert np.array_equal(np.asarray(p, dtype=np.float32), want["policy"][seed]), seed
        assert list(v) == list(want["value"][seed])
