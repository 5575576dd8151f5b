"""Reanalysis of stored plies, the parts that need no device: azh_samples_retarget_host against the Python restatement of the
target and value rule (tests/reanalyse_reference.py), bit for bit; training.reanalyse_plan; train.py's refusals."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import link, training
from tests import reanalyse_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS, FULL, BAD = link.SAMPLES_PLY_PASS, link.SAMPLES_PLY_FULL, link.SAMPLES_PLY_BAD


def _same(record, what):
    index, weight, value = link.retarget_host(record)
    want_index, want_weight, want_value = ref.retarget(record)
    assert index.dtype == np.uint16 and weight.dtype == np.float32
    assert index.tobytes() == want_index.tobytes(), what
    assert weight.tobytes() == want_weight.tobytes(), what
    assert np.float64(value).tobytes() == np.float64(want_value).tobytes(), what
    return index, weight, value


def test_the_restatement_and_the_library_agree_on_every_shape():
    records, names = ref.shaped_records(np.random.default_rng(11), 17 * 6)
    seen = {}
    for rec, name in zip(records, names):
        index, weight, value = _same(rec, name)
        seen.setdefault(name, []).append((rec, index, weight, value))
    assert set(seen) >= {"M=1", "M=63", "M=64", "M=65", "M=256", "single", "last round", "ties", "total=0", "finished",
                         "W=nan", "W=inf", "heavy"}
    for name in ("total=0", "finished", "M=0"):                     # the ply stays as it was
        assert all(len(i) == 0 and v == 0.0 for _, i, _, v in seen[name]), name
    for name in ("W=nan", "W=inf", "W=-inf"):                       # a q that is not finite reads 0
        assert all(len(i) > 0 and v == 0.0 for _, i, _, v in seen[name]), name
    for rec, index, weight, _ in seen["single"]:
        assert len(index) == 1 and weight[0] == 1.0
    for rec, index, weight, _ in seen["last round"]:
        visited = np.flatnonzero(rec[5:5 + 4 * 256:4])
        assert visited.min() >= 192 and len(index) == len(visited)
    for rec, index, weight, _ in seen["heavy"]:
        assert len(index) == 256 and int(rec[5:5 + 4 * 256:4].max()) == 65535
    assert any(v not in (0.0, -1.0, 1.0) for _, _, _, v in seen["plain"])
    for name, rows in seen.items():                                 # every changed target sums to one as the store asks
        for _, index, weight, _ in rows:
            if len(index):
                assert abs(1.0 - float(weight.astype(np.float64).sum())) < 1e-3 and len(set(index.tolist())) == len(index), name


def test_the_first_of_the_most_visited_edges_gives_the_value():
    moves = ref.MOVES[:6]
    rec = ref.record(moves, [3, 9, 2, 9, 9, 0], [0.0, 2.25, 0.0, 9.0, 0.0, 0.0])
    _, _, value = _same(rec, "tie")
    assert value == 2.0 * float(np.float32(2.25) / np.float32(9)) - 1.0 == -0.5


def test_malformed_records_are_refused():
    for rec in ref.malformed_records(np.random.default_rng(5)):
        with pytest.raises(ref.Malformed):
            ref.retarget(rec)
        with pytest.raises(link.AzhError) as err:
            link.retarget_host(rec)
        assert "error -2" in str(err.value)
    rec = ref.record([49 | 49 << 8, ref.MOVES[0]], [0, 4], [0.0, 1.0])     # an unvisited edge's move is not read
    index, _, _ = _same(rec, "unvisited")
    assert len(index) == 1


# ---------------------------------------------------------------- the plan

def _mirror(rng):
    """40 games on three wall maps: with and without "full", with passes, BAD plies, and games without a candidate."""
    games, flags, cand, count, masks = [], [], [], [], []
    for g in range(40):
        plies = int(rng.integers(1, 30))
        has_full = g % 3 == 1
        f = np.zeros(plies, dtype=np.uint8)
        f[rng.random(plies) < 0.1] |= PASS
        f[rng.random(plies) < 0.1] |= BAD
        if has_full:
            f[rng.random(plies) < 0.4] |= FULL
            if g == 7:
                f &= ~np.uint8(FULL)
        mine = [p for p in range(plies) if not has_full or f[p] & FULL]
        games.append((len(flags), plies, 1 | (link.SAMPLES_GAME_HAS_FULL if has_full else 0), 0))
        cand += mine + [0] * (plies - len(mine))
        count.append(len(mine))
        flags += f.tolist()
        masks.append((0, 1 << 24, (1 << 17) | (1 << 31))[int(rng.integers(3))])
    return (np.array(games, dtype=np.uint32), np.array(flags, dtype=np.uint8), np.array(cand, dtype=np.uint16),
            np.array(count, dtype=np.uint32), np.array(masks, dtype=np.uint64))


def _eligible(games, flags, cand, count, first_game, n_games):
    out = set()
    for g in range(first_game, first_game + n_games):
        first = int(games[g][0])
        for k in range(int(count[g])):
            p = int(cand[first + k])
            if not flags[first + p] & (PASS | BAD):
                out.add((g, p))
    return out


@pytest.mark.parametrize("fraction, slots", [(0.0, 8), (0.3, 8), (0.5, 1), (0.77, 16), (1.0, 4096)])
def test_plan(fraction, slots):
    games, flags, cand, count, masks = _mirror(np.random.default_rng(2))
    eligible = _eligible(games, flags, cand, count, 10, 30)
    assert len(eligible) > 100
    random.seed(99)
    state = random.getstate()
    plan = training.reanalyse_plan(games, flags, cand, count, masks, 10, 30, fraction, slots, seed=5)
    assert random.getstate() == state                                # the global generator is not touched
    picked = [(int(g), int(p)) for _, rows in plan for g, p in rows]
    assert len(picked) == round(fraction * len(eligible))
    assert len(set(picked)) == len(picked) and set(picked) <= eligible
    assert all(g >= 10 for g, _ in picked)
    keys = [(mask, int(g), int(p)) for mask, rows in plan for g, p in rows]
    assert keys == sorted(keys)
    for mask, rows in plan:
        assert 1 <= len(rows) <= slots and rows.dtype == np.int32 and rows.shape[1] == 2
        assert all(int(masks[g]) == mask for g, _ in rows)
    for (m0, r0), (m1, _) in zip(plan, plan[1:]):                    # a round is cut short only where the mask changes
        assert len(r0) == slots or m0 != m1
    again = training.reanalyse_plan(games, flags, cand, count, masks, 10, 30, fraction, slots, seed=5)
    assert [(m, r.tolist()) for m, r in again] == [(m, r.tolist()) for m, r in plan]
    if 0.0 < fraction < 1.0:
        other = training.reanalyse_plan(games, flags, cand, count, masks, 10, 30, fraction, slots, seed=6)
        assert [(m, r.tolist()) for m, r in other] != [(m, r.tolist()) for m, r in plan]


def test_plan_refuses_what_it_cannot_serve():
    games, flags, cand, count, masks = _mirror(np.random.default_rng(2))
    for fraction, slots, first, n in ((-0.1, 8, 10, 30), (1.5, 8, 10, 30), (0.5, 0, 10, 30), (0.5, 8, 20, 30)):
        with pytest.raises(ValueError):
            training.reanalyse_plan(games, flags, cand, count, masks, first, n, fraction, slots, seed=1)


def test_the_kl_of_two_targets():
    start = np.array([0, 2, 3], dtype=np.int32)
    old = (start, np.array([5, 9, 7], dtype=np.uint16), np.array([0.5, 0.5, 1.0], dtype=np.float32))
    new = (start, np.array([9, 5, 8], dtype=np.uint16), np.array([0.25, 0.75, 1.0], dtype=np.float32))
    got = training.target_kl(old, new)
    want = [ref.kl(old[1][:2], old[2][:2], new[1][:2], new[2][:2]), ref.kl(old[1][2:], old[2][2:], new[1][2:], new[2][2:])]
    assert np.allclose(got, want, rtol=1e-12) and got[0] > 0 and got[1] > 20


# ---------------------------------------------------------------- train.py

@pytest.mark.parametrize("flags", [["--reanalyse-fraction", "0.5", "--reanalyse-visits", "8"],
                                   ["--reanalyse-fraction", "1.5", "--reanalyse-visits", "8", "--old-path", "old.npy"],
                                   ["--reanalyse-fraction", "-0.5", "--reanalyse-visits", "8", "--old-path", "old.npy"],
                                   ["--reanalyse-fraction", "0.5", "--reanalyse-visits", "0", "--old-path", "old.npy"],
                                   ["--reanalyse-fraction", "0.5", "--old-path", "old.npy"]])
def test_train_cli_refusals(flags, tmp_path):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--games", str(tmp_path / "none.json"), "--new-path",
                          str(tmp_path / "new.npy")] + flags, cwd=ROOT, capture_output=True, timeout=300)
    assert res.returncode != 0
    assert "--reanalyse-fraction takes F in [0, 1]" in res.stderr.decode() and "--old-path" in res.stderr.decode()
    assert not os.path.exists(tmp_path / "new.npy")


def test_train_refuses_in_the_library_call_too(tmp_path):
    for kwargs in ({"reanalyse_fraction": 0.5, "reanalyse_visits": 8, "old_path": None},
                   {"reanalyse_fraction": 1.5, "reanalyse_visits": 8, "old_path": "old.npy"},
                   {"reanalyse_fraction": 0.5, "reanalyse_visits": 0, "old_path": "old.npy"}):
        old = kwargs.pop("old_path")
        with pytest.raises(ValueError) as err:
            training.train([str(tmp_path / "none.json")], old, str(tmp_path / "new.npy"), **kwargs)
        assert "--reanalyse" in str(err.value)
