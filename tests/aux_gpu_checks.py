"""The device checks of tests/test_gpu_aux_targets.py, run in a process of their own for the reason tests/samples_gpu_checks.py
gives: `python -m tests.aux_gpu_checks OUT.json` runs every check and writes {name: "ok" | traceback}; after a check that ends
in a device error nothing more is run.  Stores of at most a dozen games, launches of at most 130 samples."""
import json
import random

import numpy as np
import torch

from ataxxzero_amd import link, training
from tests import aux_fixtures as fx
from tests import fresh_process
from tests import walls_fixtures as wf
from tests.store_checks import host, move_text, restated, same, store_of

F32 = np.float32
PASS, FULL = link.SAMPLES_PLY_PASS, link.SAMPLES_PLY_FULL


def parity_entries():
    walled = fx.walled_games()
    golden = fx.golden_entries()[1]                      # one empty cell, handed to the side not to move
    return [golden, walled[3][0], fx.cut(walled[4][0]), fx.cut(walled[2][0], 1)]


def every_symmetry_and_mover(entries):
    """Per symmetry the draws of plies 0, 1, 6, 7, the two last but one and the last of every game (where it has them)."""
    for s in range(8):
        draws = []
        for g, e in enumerate(entries):
            n = len(e["boards"])
            draws += [(g, p, s) for p in sorted({0, 1, 6, 7, n - 3, n - 2, n - 1}) if 0 <= p < n]
        assert len(draws) <= 130 and {p % 2 for _, p, _ in draws} == {0, 1}
        yield draws


# ---------------------------------------------------------------- the checks

def check_parity_from_game_lines():
    entries = parity_entries()
    arrays = link.entries_to_arrays(entries, aux=True)
    assert arrays.owners[:2].all() and not arrays.owners[2:].any() and arrays.blockers[1] and not arrays.blockers[0]
    store = store_of(arrays)
    assert store.game_owners().tobytes() == arrays.owners.tobytes()
    seen = set()
    for draws in every_symmetry_and_mover(entries):
        got = host(store.gather(draws, aux=True))
        want = restated(entries, draws)
        same(got, want, draws[0][2])
        i = next(k for k, d in enumerate(draws) if d[0] == 1)
        seen.add(got[3][i].tobytes())
        for k, (g, _, _) in enumerate(draws):
            assert got[6][k, 0] == (1.0 if g < 2 else 0.0)
        assert got[6][[k for k, (g, p, _) in enumerate(draws) if p == len(entries[g]["boards"]) - 1], 1].max() == 0.0
        assert got[6][:, 1].max() == 1.0
    assert len(seen) == 8                                # the asymmetric wall map: eight different ownership images
    # and the trainer's own path: the host pipeline's draws, bit for bit its seven arrays
    random.seed(3)
    want = training.make_minibatch_reference(entries, 130, 0.0, aux=True)
    random.seed(3)
    same(host(training.make_minibatch_device(store, 0, len(entries), 130, aux=True)), want)
    store.close()


def check_parity_from_records():
    asym = link.cells_to_blockers(wf.ASYMMETRIC_CELLS)
    store = link.SampleStore(8, 2000, 20000)
    entries = []
    for fen, mask in ((wf.PLAIN_FEN, 0), (wf.ASYMMETRIC_FEN, asym)):
        games = fx.passless_games(fen, 2)
        recs = [fx.record_of(e, positions, uid) for uid, (e, positions) in enumerate(games)]
        recs.append(fx.record_of(fx.cut(games[1][0]), games[1][1][:fx.PLIES_CUT], 2))
        store.add_records(np.concatenate(recs), mask, aux=True)
        entries += [json.loads(link.format_record_json(r, blockers=mask if mask else None)) for r in recs]
    owners = store.game_owners()
    assert owners[[0, 1, 3, 4]].all() and not owners[[2, 5]].any()
    assert [int(m) for m in store.game_blockers()] == [0, 0, 0, asym, asym, asym]
    for draws in every_symmetry_and_mover(entries):
        same(host(store.gather(draws, aux=True)), restated(entries, draws), draws[0][2])
    entry, positions = fx.passless_games(wf.PLAIN_FEN, 1)[0]
    bad = fx.record_of(entry, positions)
    at = len(bad) - len(entry["dists"][-1]) - 2                       # the last ply's move | nd << 16
    bad[at] = (int(bad[at]) & 0xFFFF0000) | 0x3131                     # a move to square 49
    counts = store.counts()
    try:
        store.add_records(bad, 0, aux=True)
    except link.AzhError as err:
        assert "error -2" in str(err), err
    else:
        raise AssertionError("a record with an illegal last move was accepted")
    assert store.counts() == counts
    store.close()


def check_parity_of_the_existing_outputs():
    entries = fx.mixed_entries()[:12]
    store = store_of(link.entries_to_arrays(entries, aux=True))
    rng = np.random.default_rng(5)
    draws = []
    while len(draws) < 130:
        g = int(rng.integers(len(entries)))
        p = int(rng.integers(len(entries[g]["boards"])))
        if entries[g]["moves"][p] != "pass":
            draws.append((g, p, int(rng.integers(8))))
    for blend in (0.0, 0.5):
        same(host(store.gather(draws, blend, aux=True))[:3], host(store.gather(draws, blend)))
    plain_draws = torch.zeros((130, 4), dtype=torch.int32, device="cuda")
    aux_draws = torch.full((130, 4), 7, dtype=torch.int32, device="cuda")
    for step in range(3):
        plain = host(store.draw_gather(130, 99, step, 2, 10, 0.5, draws_out=plain_draws))
        with_aux = host(store.draw_gather(130, 99, step, 2, 10, 0.5, draws_out=aux_draws, aux=True))
        same(with_aux[:3], plain)
        assert torch.equal(plain_draws, aux_draws)
    assert store.status() == 0
    store.close()


def hand_built(target_counts, flags, game_word=1, rng=None, weights=None):
    """One game of len(target_counts) plies as SampleArrays: ply p has target_counts[p] targets on distinct policy cells."""
    rng = rng or np.random.default_rng(9)
    n = len(target_counts)
    boards = np.zeros((n, 2), dtype=np.uint64)
    for p in range(n):
        cells = rng.integers(0, 3, size=49)
        boards[p] = [sum(1 << i for i in range(49) if cells[i] == v) for v in (1, 2)]
    index, weight, start = [], [], [0]
    for p, k in enumerate(target_counts):
        index.append(rng.choice(833, size=k, replace=False).astype(np.uint16))
        w = rng.dirichlet(np.ones(k)).astype(F32) if k else np.zeros(0, F32)
        weight.append(w * (weights[p] if weights else 1.0))
        start.append(start[-1] + k)
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    return (np.array([[0, n, game_word, 0]], dtype=np.uint32), boards, np.array(flags, dtype=np.uint8), np.zeros(n),
            np.array(start, dtype=np.int32), cat(index, np.uint16), cat(weight, F32))


def scattered(arrays, ply, s):
    """Ply `ply`'s target under symmetry s as a (7, 7, 17) array: every weight alone on its cell."""
    lo, hi = arrays.target_start[ply], arrays.target_start[ply + 1]
    out = np.zeros(833, dtype=F32)
    for i, w in zip(arrays.target_index[lo:hi], arrays.target_weight[lo:hi]):
        cell = link.symmetry_policy_index(s, int(i))
        assert out[cell] == 0
        out[cell] = w
    return out.reshape(7, 7, 17)


def check_edges_of_the_wave_for_the_reply_scatter():
    counts = [2, 1, 63, 64, 65, 833]
    arrays = link.SampleArrays(*hand_built(counts, [0] * 6), owners=np.zeros((1, 2), np.uint64))
    store = store_of(arrays)
    assert store.counts()["bad_plies"] == 0
    _, policy_to = training._symmetry_tables()
    real = [training._flat_policy_index(move_text(a | b << 8)) for a in range(49) for b in range(49)
            if a == b or max(abs(a % 7 - b % 7), abs(a // 7 - b // 7)) == 2]
    assert len(set(real)) == 529
    for s in range(8):
        for i in real:                                    # the map `scattered` uses is the trainer's on every real move
            assert policy_to[s, i] == link.symmetry_policy_index(s, i), (s, i)
        got = host(store.gather([(0, p, s) for p in range(6)], aux=True))
        for p in range(6):
            assert got[1][p].tobytes() == scattered(arrays, p, s).tobytes(), (s, p)
            want = scattered(arrays, p + 1, s) if p < 5 else np.zeros((7, 7, 17), F32)
            assert got[5][p].tobytes() == want.tobytes(), (s, p)
            assert np.count_nonzero(got[5][p]) == (counts[p + 1] if p < 5 else 0)
        assert got[6].tolist() == [[0.0, 1.0]] * 5 + [[0.0, 0.0]]
        assert not got[3].any() and not got[4].any()
    store.close()


def check_reply_absent():
    # no "full": ply 1 is a pass, ply 3 is bad (its weights sum to a half), ply 4 is the last
    plain = link.SampleArrays(*hand_built([3, 0, 5, 4, 6], [0, PASS, 0, 0, 0], weights=[1, 1, 1, 0.5, 1]),
                              owners=np.zeros((1, 2), np.uint64))
    # "full": plies 0, 2 and 3 were searched in full
    capped = link.SampleArrays(*hand_built([3, 4, 5, 6], [FULL, 0, FULL, FULL], game_word=2 | link.SAMPLES_GAME_HAS_FULL),
                               owners=np.zeros((1, 2), np.uint64))
    for arrays, draws, present in ((plain, [0, 2, 4], [0, 0, 0]), (capped, [0, 1, 2, 3], [0, 1, 1, 0])):
        store = store_of(arrays)
        got = host(store.gather([(0, p, 5) for p in draws], aux=True))
        assert got[6][:, 1].tolist() == [float(v) for v in present]
        for row, p, has in zip(got[5], draws, present):
            assert row.tobytes() == (scattered(arrays, p + 1, 5) if has else np.zeros((7, 7, 17), F32)).tobytes(), p
        store.close()
    store = store_of(plain)
    assert store.counts()["bad_plies"] == 1
    store.close()


def check_device_draws_with_aux():
    mixed = fx.mixed_entries()
    undrawable = [dict(e, full=[0] * len(e["boards"])) for e in (fx.cut(mixed[6]), fx.cut(mixed[9], 7))]
    entries = undrawable + mixed[2:8] + mixed[12:16]      # golden and walled games, cuts without owners, games with "full"
    assert len(entries) == 12
    store = store_of(link.entries_to_arrays(entries, aux=True))
    n = 130
    draws_out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    weights = np.zeros(2)
    for step in range(2):
        got = host(store.draw_gather(n, 77, step, 2, 10, 0.0, draws_out=draws_out, aux=True))
        draws = draws_out.cpu().numpy()
        for i in range(n):
            assert tuple(int(v) for v in draws[i]) == store.draw(77, step, i, 2, 10), (step, i)
        same(got, restated(entries, draws[:, :3].tolist()), step)
        weights += got[6].sum(axis=0)
    assert (weights > 0).all() and (weights < 2 * n).all() and store.status() == 0
    out = store.aux_outputs(n)
    for t in out:
        t.fill_(7.0)
    store.draw_gather(n, 77, 0, 0, 2, 0.0, out=out, draws_out=draws_out, aux=True)      # a range of undrawable games
    assert store.status() == n
    assert all(float(t.abs().max()) == 0.0 for t in out)
    assert (draws_out.cpu().numpy() == np.array([-1, -1, -1, 64])).all()
    store.close()


def check_stale_rows():
    entries = parity_entries()
    store = store_of(link.entries_to_arrays(entries, aux=True))
    last = [len(e["boards"]) - 1 for e in entries]
    first = [(0, 2, 1), (1, 3, 2), (1, last[1] - 1, 3), (0, 5, 4)] * 16          # owners and a reply in every row
    second = [(2, 4, 1), (3, 0, 2), (2, last[2], 3), (0, last[0], 4)] * 16       # no owners, no reply, neither, no reply
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                                  # torch's current stream
        out = store.aux_outputs(len(first))
        store.gather(first, aux=True, out=out)
        kept = [t.clone() for t in out]
        store.gather(second, aux=True, out=out)
    side.synchronize()
    got_first, got_second = host(kept), host(out)
    assert got_first[6].min() == 1.0
    assert got_second[6][:4].tolist() == [[0.0, 1.0], [0.0, 0.0], [0.0, 0.0], [1.0, 0.0]]
    same(got_first, restated(entries, first))
    same(got_second, restated(entries, second))
    assert not got_second[3][:3].any() and not got_second[5][1:4].any()
    store.close()


def check_no_owners_anywhere():
    entries = [fx.cut(e, 12) for e, _ in fx.walled_games()[:4]]
    draws = [(g, p, (g + p) % 8) for g in range(4) for p in range(12)]
    want = restated(entries, draws)
    assert not want[6][:, 0].any() and want[6][:, 1].any()
    for arrays in (link.entries_to_arrays(entries), link.entries_to_arrays(entries, aux=True)):     # no owners given; all zero
        store = store_of(arrays)
        assert not store.game_owners().any()
        same(host(store.gather(draws, aux=True)), want)
        got = host(store.draw_gather(64, 5, 0, 0, 4, aux=True))
        assert not got[6][:, 0].any() and not got[3].any() and not got[4].any() and got[6][:, 1].any()
        store.close()


def check_ingest_refusals():
    entries = parity_entries()[:2]
    good = link.entries_to_arrays(entries, aux=True)
    store = store_of(link.entries_to_arrays(entries[:1], aux=True), spare=len(good.target_index) + 500)
    counts, owners = store.counts(), store.game_owners().copy()
    walls = int(good.blockers[1])
    x, o = (int(v) for v in good.owners[1])
    cell = next(b for b in range(49) if x >> b & 1)
    wall = next(b for b in range(49) if walls >> b & 1)
    swapped = [o, x] if bin(x).count("1") != bin(o).count("1") else None
    assert swapped is not None
    for what, pair in (("overlap", [x, o | 1 << cell]), ("a wall", [x | 1 << wall, o]), ("bit 49", [x | 1 << 49, o]),
                       ("unowned", [x & ~(1 << cell), o]), ("margin", swapped)):
        bad = link.entries_to_arrays(entries, aux=True)
        bad.owners[1] = pair
        try:
            store.add_arrays(bad)
        except link.AzhError as err:
            assert "error -2" in str(err) and "game 1" in str(err), (what, err)
        else:
            raise AssertionError("owners with %s were accepted" % what)
        assert store.counts() == counts and store.game_owners().tobytes() == owners.tobytes(), what
    store.add_arrays(good)                                 # and the good ones go in
    assert store.counts()["games"] == 3 and store.game_owners()[1:].tobytes() == good.owners.tobytes()
    store.close()


CHECKS = [check_parity_from_game_lines, check_parity_from_records, check_parity_of_the_existing_outputs,
          check_edges_of_the_wave_for_the_reply_scatter, check_reply_absent, check_device_draws_with_aux, check_stale_rows,
          check_no_owners_anywhere, check_ingest_refusals]


if __name__ == "__main__":
    fresh_process.main(CHECKS)
