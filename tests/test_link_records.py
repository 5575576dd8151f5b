"""link.records, the one Python walk of the finished-game record (csrc/record.h), against the lines the library writes for the
same words (link.format_record_json) — checked on the CPU, no device needed."""
import itertools
import json

import numpy as np
import pytest

from ataxxzero_amd import link
from tests.record_fixtures import move_name, random_record, random_records

MODE_BITS = (link.REC_KIND_PLAYOUT_CAP, link.REC_KIND_FORCED, link.REC_KIND_VALUES, link.REC_KIND_RESIGNED)
# every kind word azh_format_record_json takes: a whole game or one begun at a loaded position, beside any of the mode bits
# (the Gumbel bit is formatted by the engine's drain alone: checked below against the same record without it)
KINDS = [low | sum(bits) for low in (link.REC_KIND_WHOLE, link.REC_KIND_LOADED)
         for n in range(len(MODE_BITS) + 1) for bits in itertools.combinations(MODE_BITS, n)]


def _with_kind(rec, kind, rng):
    """the record with its kind word set and word 5 of every ply written as the kind's modes write it"""
    rec = rec.copy()
    rec[link.REC_KIND] = kind
    at = link.REC_HDR_WORDS
    for _ in range(int(rec[link.REC_PLIES])):
        full = int(rng.integers(0, 2))
        if kind & link.REC_KIND_VALUES:
            q = np.array([rng.random()], dtype=np.float32).view(np.uint32)[0]
            rec[at + 5] = (int(q) & link.REC_PLY_Q_BITS) | (full * link.REC_PLY_FULL_BIT)
        elif kind & link.REC_KIND_PLAYOUT_CAP:
            rec[at + 5] = full
        at += link.REC_PLY_WORDS + (int(rec[at + 4]) >> 16)
    return rec


def _check_against_the_line(rec):
    (r,) = link.records(rec)
    entry = json.loads(link.format_record_json(rec, with_ids=True))
    assert (r.slot, r.uid, r.result) == (entry["slot"], entry["uid"], entry["result"])
    assert r.kind == int(rec[link.REC_KIND]) and r.words.tobytes() == rec.tobytes()
    assert len(r.plies) == len(entry["boards"]) == len(entry["moves"]) == len(entry["dists"])
    assert [move_name(m & 0xFF, m >> 8) for m, _, _, _ in r.plies] == entry["moves"]
    assert [{move_name(m & 0xFF, m >> 8) for m in counts} for _, _, counts, _ in r.plies] == [set(d) for d in entry["dists"]]
    for (_, _, _, (x, o)), board in zip(r.plies, entry["boards"]):
        assert [1 if x >> (c % 7 + 7 * (6 - c // 7)) & 1 else 2 if o >> (c % 7 + 7 * (6 - c // 7)) & 1 else 0
                for c in range(49)] == board
    valued = bool(r.kind & link.REC_KIND_VALUES)
    assert ("full" in entry) == bool(r.kind & link.REC_KIND_PLAYOUT_CAP)
    if "full" in entry:
        assert entry["full"] == [int(bool(w5 & link.REC_PLY_FULL_BIT if valued else w5)) for _, w5, _, _ in r.plies]
    assert len(entry.get("values", [])) == (len(r.plies) if valued else 0) and ("values" in entry) == valued
    assert ("resigned" in entry) == bool(r.kind & link.REC_KIND_RESIGNED)
    assert entry.get("random_ply", -1) == int(rec[link.REC_RANDOM_PLY_PLUS_1]) - 1


def test_parsed_records_reproduce_their_lines_over_every_kind():
    rng = np.random.default_rng(11)
    records, entries = random_records()
    assert any("random_ply" in e for e in entries) and any("random_ply" not in e for e in entries)
    for i, rec in enumerate(records):
        _check_against_the_line(_with_kind(rec, KINDS[i % len(KINDS)], rng))
    assert len(records) >= 2 * len(KINDS) and len(KINDS) == 32
    for kind in KINDS:                                            # every kind with and without random_ply
        for random_ply in (None, 5):
            rec, _ = random_record(rng, plies=7, visits_hi=400, random_ply=random_ply)
            _check_against_the_line(_with_kind(rec, kind, rng))


@pytest.mark.parametrize("nd", [0, 1, 256])
def test_plies_with_no_target_one_target_and_the_most_a_ply_holds(nd):
    rng = np.random.default_rng(nd)
    assert link.REC_MAXD == 256
    for kind in KINDS:
        rec, _ = random_record(rng, plies=3, visits_hi=255, targets=nd)
        rec = _with_kind(rec, kind, rng)
        _check_against_the_line(rec)
        assert [len(counts) for _, _, counts, _ in next(link.records(rec)).plies] == [nd] * 3


def test_the_gumbel_bit_changes_the_kind_word_alone():
    rng = np.random.default_rng(3)
    rec, _ = random_record(rng, plies=9, visits_hi=65535)
    gumbel = rec.copy()
    gumbel[link.REC_KIND] |= link.REC_KIND_GUMBEL
    (a,), (b,) = link.records(rec), link.records(gumbel)
    assert b.kind == a.kind | link.REC_KIND_GUMBEL and b[:3] == a[:3] and b.plies == a.plies
    assert link.REC_KIND_MODES == sum(MODE_BITS) + link.REC_KIND_GUMBEL


def test_a_truncated_record_and_a_wrong_magic_raise():
    rng = np.random.default_rng(5)
    rec, _ = random_record(rng, plies=4, visits_hi=50)
    assert len(list(link.records(rec))) == 1
    bad = rec.copy()
    bad[link.REC_MAGIC] ^= 1
    for words in (bad, rec[:-1], rec[:link.REC_HDR_WORDS + 3], rec[:5]):
        with pytest.raises(AssertionError):
            list(link.records(words))
    cut = rec.copy()
    cut[link.REC_PLIES] += 1                       # one ply more than the words hold
    slack = np.concatenate([rec, np.zeros(3, dtype=np.uint32)])
    slack[link.REC_WORDS] += 3                     # the plies do not fill the record
    for words in (cut, slack):
        with pytest.raises(AssertionError):
            list(link.records(words))


def test_several_records_with_a_dropped_games_marker_between_them():
    rng = np.random.default_rng(8)
    recs = [random_record(rng, plies=int(rng.integers(1, 9)), visits_hi=100, uid=uid)[0] for uid in (4, 6, 9)]
    marker = np.array([link.RECORD_MAGIC, 2, 5, 17, 0, link.REC_HDR_WORDS, 0, link.REC_KIND_DROPPED], dtype=np.uint32)
    words = np.concatenate([recs[0], marker, recs[1], recs[2]])
    assert [r.uid for r in link.records(words)] == [4, 6, 9]
    with_markers = list(link.records(words, markers=True))
    assert [r.uid for r in with_markers] == [4, 5, 6, 9]
    assert with_markers[1].kind == link.REC_KIND_DROPPED and with_markers[1].plies == [] and \
        with_markers[1].words.tobytes() == marker.tobytes()
    assert b"".join(r.words.tobytes() for r in with_markers) == words.tobytes()
    assert list(link.records(words[:0])) == []
