"""Walls through the loop, the parts that need no device: the FEN round trip of uai.Position, the game line's "blockers" key,
feature plane 3 in the host sample pipeline, the refusals of malformed wall lists, the record path with a mask, and the masked
legal-move list and surprise of the store's host restatements."""
import ctypes
import json
import random

import numpy as np
import pytest

from ataxxzero_amd import link, selfplay, training, uai
from tests import rules_reference as rr
from tests import surprise_reference as ref
from tests import walls_fixtures as wf
from tests.samples_fixtures import _arrays_equal, random_record

F32 = np.float32
FENS = [wf.DEFAULT_FEN, wf.ASYMMETRIC_FEN, "x5o/7/3-3/2-1-2/3-3/7/o5x o", "-------/-------/7/7/7/7/xo5 x"]


# ---------------------------------------------------------------- 1. FEN

@pytest.mark.parametrize("fen", FENS + [wf.PLAIN_FEN])
def test_position_keeps_the_walls_of_a_fen(fen):
    x, o, walls, turn = selfplay.parse_fen(fen)
    pos = uai.Position.from_fen(fen)
    assert (pos.x, pos.o, pos.blockers, pos.turn) == (x, o, walls, turn)
    assert pos.fen() == fen and selfplay.parse_fen(pos.fen()) == (x, o, walls, turn)
    assert pos.fen() == rr.Board.from_fen(fen).fen()                 # the third statement of the dialect writes the same text
    assert pos == uai.Position.from_fen(fen) and pos == pos.copy()
    if walls:
        assert pos != uai.Position(x, o, turn) and "-" in pos.fen() and "-" in str(pos)
    else:
        assert pos == uai.Position(x, o, turn) and "-" not in pos.fen()


# ---------------------------------------------------------------- 2. the line

def _record(seed, mask, kind=0):
    """A record whose stones keep off the cells of `mask`."""
    rec = random_record(np.random.default_rng(seed), 5, 400, kind=kind, uid=seed)
    at = 8
    for _ in range(int(rec[3])):
        rec[at] &= ~mask & 0xFFFFFFFF
        rec[at + 1] &= ~(mask >> 32) & 0xFFFFFFFF
        rec[at + 2] &= ~mask & 0xFFFFFFFF
        rec[at + 3] &= ~(mask >> 32) & 0xFFFFFFFF
        at += 6 + (int(rec[at + 4]) >> 16)
    return rec


@pytest.mark.parametrize("fen,cells", [(wf.DEFAULT_FEN, [17, 23, 25, 31]), (wf.PLAIN_FEN, []),
                                       (wf.ASYMMETRIC_FEN, wf.ASYMMETRIC_CELLS)])
def test_the_line_with_blockers_is_the_line_without_plus_the_key(fen, cells):
    mask = selfplay.parse_fen(fen)[2]
    assert link.blockers_to_cells(mask) == cells and link.cells_to_blockers(cells) == mask
    for kind in (0, 4, 16, 4 | 16 | 32):
        for with_ids in (False, True):
            rec = _record(3 + kind, mask, kind)
            plain = link.format_record_json(rec, with_ids)
            keyed = link.format_record_json(rec, with_ids, blockers=mask)
            key = b'"blockers":' + json.dumps(cells, separators=(",", ":")).encode() + b","
            assert keyed == plain[:1] + key + plain[1:]                  # the key leads the object; its bytes removed: the old line
            entry = json.loads(keyed)
            assert entry["blockers"] == cells and list(entry)[0] == "blockers" and list(entry) == sorted(entry)
            del entry["blockers"]
            assert entry == json.loads(plain)
    with pytest.raises(link.AzhError):
        link.format_record_json(_record(1, 0), blockers=1 << 49)


# ---------------------------------------------------------------- 3. the minibatch

def test_minibatch_shows_the_walls_in_plane_three():
    entries, _ = wf.mixed_entries()
    assert [e.get("blockers") for e in entries] == [[17, 23, 25, 31], None, wf.ASYMMETRIC_CELLS, wf.ASYMMETRIC_CELLS,
                                                    [17, 23, 25, 31], None]
    stripped = [{k: v for k, v in e.items() if k != "blockers"} for e in entries]
    for seed in range(3):
        random.seed(seed)
        want = training.make_minibatch_reference(entries, 96)
        state = random.getstate()
        random.seed(seed)
        got = training.make_minibatch(entries, 96)
        assert random.getstate() == state
        for g, w in zip(got, want):
            assert g.dtype == w.dtype == F32 and g.tobytes() == w.tobytes()
        # the draws are the ones the same games without the key consume, and everything but plane 3 is what they give
        random.seed(seed)
        bare = training.make_minibatch(stripped, 96)
        assert random.getstate() == state
        random.seed(seed)
        bare_reference = training.make_minibatch_reference(stripped, 96)
        assert random.getstate() == state
        assert (bare[0][..., 3] == 0).all() and (bare_reference[0][..., 3] == 0).all()
        assert (bare[0][..., :3] == got[0][..., :3]).all() and (bare[1] == got[1]).all() and (bare[2] == got[2]).all()
        assert (got[0][..., 3] != 0).any() and (got[0][..., 3].sum(axis=(1, 2)) == 0).any()      # walled and unwalled samples
        assert not ((got[0][..., 3] != 0) & ((got[0][..., 1] != 0) | (got[0][..., 2] != 0))).any()   # never a stone on a wall


def test_plane_three_of_every_symmetry_and_both_movers():
    for fen, cells in ((wf.DEFAULT_FEN, [17, 23, 25, 31]), (wf.ASYMMETRIC_FEN, wf.ASYMMETRIC_CELLS)):
        entry, _ = wf.games(fen, 2)[0]
        images = set()
        for ply in (0, 1):
            mover = 1 + ply % 2
            plain = training.board_to_features(entry["boards"][ply], mover)
            feats = training.board_to_features(entry["boards"][ply], mover, entry["blockers"])
            assert (feats[..., :3] == plain[..., :3]).all() and (plain[..., 3] == 0).all()
            assert (feats[..., 3:] == wf.wall_plane(cells)).all()
            for s in range(8):
                image = training.apply_symmetry(s, feats)
                assert (image[..., 3:] == training.apply_symmetry(s, wf.wall_plane(cells))).all()
                images.add(image[..., 3].tobytes())
        assert len(images) == (1 if fen == wf.DEFAULT_FEN else 8)        # the asymmetric map: every symmetry moves it
    # through the batched pipeline: sample i's plane 3 is the symmetry the i-th draw made, applied to the wall plane
    entry, _ = wf.games(wf.ASYMMETRIC_FEN, 2)[0]
    seen = set()
    for seed in range(6):
        random.seed(seed)
        feats, _, _ = training.make_minibatch([entry], 32)
        random.seed(seed)
        for i in range(32):
            random.choice([entry])
            while True:
                ply = training._draw_ply(entry)
                if entry["moves"][ply] != "pass":
                    break
                random.choice([entry])
            s = random.randrange(8)
            seen.add((s, ply % 2))
            assert (feats[i, :, :, 3:] == training.apply_symmetry(s, wf.wall_plane(wf.ASYMMETRIC_CELLS))).all(), (seed, i)
    assert seen == {(s, m) for s in range(8) for m in (0, 1)}


# ---------------------------------------------------------------- 4. refusals

def _broken_entries():
    entry, _ = wf.games(wf.DEFAULT_FEN, 2)[0]
    on_a_stone = dict(entry, blockers=[entry["boards"][3].index(1)])      # a cell x holds at ply 3
    late_stone = dict(entry, blockers=[c for c in range(49) if entry["boards"][-1][c] and not entry["boards"][0][c]][:1])
    assert late_stone["blockers"]
    out = [on_a_stone, late_stone]
    for cells in ([23, 17], [17, 17], [17, 49], [-1, 3], [3.0], ["17"], "17", {"17": 1}, [True], None):
        out.append(dict(entry, blockers=cells))
    return entry, out


def test_malformed_walls_are_refused_by_name(tmp_path):
    good, broken = _broken_entries()
    training.check_blockers(good, "a game")
    training.check_blockers(dict(good, blockers=[]), "a game")
    link.entries_to_arrays([good])
    for number, entry in enumerate(broken):
        path = str(tmp_path / ("games-%d.json" % number))
        with open(path, "w") as f:
            f.write(json.dumps(good) + "\n\n" + json.dumps(entry) + "\n")
        with pytest.raises(ValueError) as err:
            training.load_entries([path])
        assert path in str(err.value) and "line 3" in str(err.value), str(err.value)
        with pytest.raises(ValueError) as err:
            link.entries_to_arrays([good, entry])
        assert "entry 1" in str(err.value)
    # the record path: a mask beyond the board, a mask under a stone — -2, nothing written
    rec = _record(5, 0)
    stone = int(rec[8]) & -int(rec[8]) or 1 << 32
    for mask in (1 << 49, stone):
        outs = [np.full(4096, 0xAB, dtype=np.uint8) for _ in range(8)]       # the seven arrays and game_blockers
        arrays = link.CSampleArrays(9, 99, 9999, *[o.ctypes.data for o in outs])
        rc = link.load().azh_samples_pack_records(rec.ctypes.data, rec.size, mask, None, 0, 0, ctypes.byref(arrays))
        assert rc == -2 and (arrays.n_games, arrays.n_plies, arrays.n_targets) == (9, 99, 9999)
        assert all((o == 0xAB).all() for o in outs)
        with pytest.raises(link.AzhError):
            link.pack_records(rec, mask)


# ---------------------------------------------------------------- 5. the record path

def test_packed_records_with_a_mask_equal_the_parse_of_their_lines():
    for fen in (wf.DEFAULT_FEN, wf.ASYMMETRIC_FEN, wf.PLAIN_FEN):
        mask = selfplay.parse_fen(fen)[2]
        recs = [_record(seed, mask, kind) for seed, kind in enumerate((0, 4, 16, 4 | 16, 16 | 32, 8))]
        packed = link.pack_records(np.concatenate(recs), mask)
        entries = [json.loads(link.format_record_json(r, blockers=mask)) for r in recs]
        parsed = link.entries_to_arrays(entries)
        _arrays_equal(packed, parsed)
        assert packed.blockers.tolist() == [mask] * len(recs) == parsed.blockers.tolist()
        unkeyed = link.entries_to_arrays([json.loads(link.format_record_json(r)) for r in recs])
        assert unkeyed.blockers.tolist() == [0] * len(recs)
        assert link.pack_records(np.concatenate(recs)).blockers.tolist() == [0] * len(recs)


# ---------------------------------------------------------------- 6. legal moves

def test_masked_legal_moves_equal_the_rules_restatement():
    counts, walled_out = set(), 0
    for fen in (wf.DEFAULT_FEN, wf.ASYMMETRIC_FEN):
        for _, positions in wf.games(fen, 6):
            for board in positions:
                mover, opponent, walls = wf.mover_view(board)
                want = [wf.policy_index(m) for m in rr.legal_moves(board)]
                assert list(link.samples_legal(mover, opponent, walls)) == want
                counts.add(len(want))
                free = list(link.samples_legal(mover, opponent))
                assert set(want) <= set(free)
                walled_out += len(free) > len(want)
    assert walled_out > 20 and max(counts) >= 30


# ---------------------------------------------------------------- 7. the surprise on the host

def test_masked_surprise_against_float64_and_against_the_unmasked_call():
    """The bound is tests/test_surprise_host.py's: what surprise_reference.kl_reference derives for the ply."""
    rng = np.random.default_rng(13)
    n = differs = reach = 0
    for fen in (wf.DEFAULT_FEN, wf.ASYMMETRIC_FEN):
        for entry, positions in wf.games(fen, 6):
            for ply, board in enumerate(positions):
                legal = [wf.policy_index(m) for m in rr.legal_moves(board)]
                if not legal:
                    continue
                mover, opponent, walls = wf.mover_view(board)
                logits = (3.0 * rng.standard_normal(833)).astype(F32)
                t_index = [training._flat_policy_index(m) for m in entry["dists"][ply]]
                t_weight = np.array(list(entry["dists"][ply].values()), dtype=F32)
                got, illegal = link.samples_surprise_host_blockers(logits, mover, opponent, walls, t_index, t_weight)
                want, want_illegal, bound = ref.kl_reference(logits, legal, t_index, t_weight)
                assert illegal == want_illegal == 0
                assert abs(float(got) - want) <= bound, (float(got), want, bound)
                assert (got, illegal) == link.samples_surprise_host(logits, legal, t_index, t_weight)
                free = link.samples_legal(mover, opponent)
                bare, _ = link.samples_surprise_host_blockers(logits, mover, opponent, 0, t_index, t_weight)
                assert (bare, 0) == link.samples_surprise_host(logits, free, t_index, t_weight)
                if len(free) > len(legal):                   # a wall cell within the mover's reach: the softmax ran over it
                    reach += 1
                    differs += bare.tobytes() != got.tobytes()
                else:
                    assert bare.tobytes() == got.tobytes()
                n += 1
    print("masked surprise: %d plies, a wall within reach on %d, the unmasked value differs on %d" % (n, reach, differs))
    assert n > 300 and reach > 50 and differs >= 1
