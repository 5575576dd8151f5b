"""The device checks of tests/test_gpu_reanalyse.py, run in a process of their own (as tests/samples_gpu_checks.py, and for its
reason: a SampleStore needs torch imported before the library is loaded).  `python -m tests.reanalyse_gpu_checks OUT.json` runs
every check and writes {name: "ok" | traceback}; after a check that ends in a device error nothing more is run."""
import json

import numpy as np
import torch

from ataxxzero_amd import link, model, selfplay, training
from tests import aux_reference as ar
from tests import fresh_process
from tests import reanalyse_reference as ref
from tests.samples_fixtures import random_record
from tests.store_checks import all_pairs, eligible_pairs, first_three, host, move_text, restated, same

F32 = np.float32
PASS, FULL, BAD = link.SAMPLES_PLY_PASS, link.SAMPLES_PLY_FULL, link.SAMPLES_PLY_BAD
PICKED = 600            # more than two workgroups of the 256-wide scan, and no multiple of it


def fixture_games(seed=7):
    """Twelve games of 64 plies as ring records: plain, with values, and two with the playout cap's "full" -> (records, their
    parsed lines, the SampleArrays of the lot)."""
    rng = np.random.default_rng(seed)
    kinds = [0, 16, 0, 16, 4 | 16, 0, 16, 0, 4, 16, 0, 0]
    recs = [random_record(rng, 64, 50, kind=kind, result=1 + uid % 2, uid=uid) for uid, kind in enumerate(kinds)]
    entries = [json.loads(link.format_record_json(r)) for r in recs]
    return recs, entries, link.pack_records(np.concatenate(recs))


def snapshot(store, pairs=None):
    """What the store holds for the plies (all of them by default), ply by ply, as bytes."""
    pairs = all_pairs(store) if pairs is None else np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    boards, values, flags, start, index, weight = store.read_plies(pairs)
    return [(boards[i].tobytes(), values[i].tobytes(), int(flags[i]), index[start[i]:start[i + 1]].tobytes(),
             weight[start[i]:start[i + 1]].tobytes()) for i in range(len(pairs))]


def upload(records):
    return torch.from_numpy(np.ascontiguousarray(records, dtype=np.uint32).view(np.int32).reshape(-1)).cuda()


def picked_call(store, rng, n=PICKED):
    """n eligible plies in a shuffled call order and a record of every shape for each."""
    pairs = eligible_pairs(store)
    assert len(pairs) >= n
    pairs = np.array([pairs[int(k)] for k in rng.choice(len(pairs), size=n, replace=False)], dtype=np.int32)
    records, names = ref.shaped_records(rng, n)
    return pairs, records, names


def apply_to_entries(entries, pairs, records, status):
    """The lines after the reanalysis: dists[ply] and values[ply] of every changed ply replaced by the restatement's."""
    for (g, p), rec, changed in zip(pairs.tolist(), records, status.tolist()):
        if not changed:
            continue
        index, weight, value = ref.retarget(rec)
        moves = [int(rec[4 + 4 * j]) for j in range(int(rec[1])) if rec[5 + 4 * j] > 0]
        assert [ref.policy_index(mv) for mv in moves] == index.tolist()
        entries[g]["dists"][p] = {move_text(mv): float(w) for mv, w in zip(moves, weight)}
        if "values" in entries[g]:
            entries[g]["values"][p] = value


# ---------------------------------------------------------------- the checks

def check_read_plies():
    recs, entries, a = fixture_games()
    store = link.SampleStore(len(a.games), len(a.ply_flags), len(a.target_index))
    store.add_arrays(a)
    pairs = all_pairs(store)
    assert len(pairs) == 12 * 64
    boards, values, flags, start, index, weight = store.read_plies(pairs)
    assert boards.tobytes() == a.boards.tobytes() and values.tobytes() == a.values.tobytes()
    assert flags.tobytes() == store.mirror()[1].tobytes() and (flags & ~np.uint8(BAD)).tobytes() == a.ply_flags.tobytes()
    assert start.tobytes() == a.target_start.tobytes()
    assert index.tobytes() == a.target_index.tobytes() and weight.tobytes() == a.target_weight.tobytes()
    assert (flags & FULL).any() and np.abs(values).max() > 0 and len(index) > 5000
    where = store.ply_targets(pairs)
    assert where[:, 0].tolist() == a.target_start[:-1].tolist() and where[:, 1].tolist() == np.diff(a.target_start).tolist()
    # a scattered list, a ply twice among it, and the call without targets
    rng = np.random.default_rng(1)
    some = np.concatenate([pairs[rng.choice(len(pairs), size=300, replace=False)], pairs[5:6], pairs[5:6]])
    got = snapshot(store, some)
    whole = snapshot(store)
    flat = {tuple(p): k for k, p in enumerate(pairs.tolist())}
    assert got == [whole[flat[tuple(p)]] for p in some.tolist()]
    b2, v2, f2, s2, i2, w2 = store.read_plies(some, targets=False)
    assert i2 is None and w2 is None and s2[-1] == sum(len(g[3]) // 2 for g in got) and b2.tobytes() == \
        store.read_plies(some)[0].tobytes()
    # refusals: a pair outside the store, room that is one target short
    for bad in ((12, 0), (0, 64), (-1, 0), (0, -1)):
        try:
            store.read_plies([bad])
        except link.AzhError as err:
            assert "error -1" in str(err), err
        else:
            raise AssertionError("pair %r was accepted" % (bad,))
    n = len(some)
    out = [np.zeros((n, 2), np.uint64), np.zeros(n), np.zeros(n, np.uint8), np.zeros(n + 1, np.int32),
           np.zeros(int(s2[-1]), np.uint16), np.zeros(int(s2[-1]), F32)]
    rc = link.load().azh_samples_read_plies(store.h, n, some.ctypes.data, *[o.ctypes.data for o in out], int(s2[-1]) - 1)
    assert rc == -6 and int(out[3][n]) == int(s2[-1])
    store.close()


def synthetic_store(spare_targets, rng):
    recs, entries, a = fixture_games()
    store = link.SampleStore(len(a.games) + 1, len(a.ply_flags) + 64, len(a.target_index) + spare_targets)
    store.add_arrays(a)
    pairs, records, names = picked_call(store, rng)
    return store, entries, a, pairs, records, names


def check_synthetic_reports():
    rng = np.random.default_rng(21)
    store, entries, a, pairs, records, names = synthetic_store(PICKED * link.MAX_MOVES, rng)
    before_all, everyone = snapshot(store), all_pairs(store)
    before = snapshot(store, pairs)
    t0 = store.counts()["targets"]
    status = store.retarget(pairs, upload(records), 0)
    after, where = snapshot(store, pairs), store.ply_targets(pairs)
    at, seen = t0, set()
    for i, (rec, name) in enumerate(zip(records, names)):
        index, weight, value = link.retarget_host(rec)
        if len(index) == 0:
            assert status[i] == 0 and after[i] == before[i], (i, name)
            continue
        seen.add(name)
        assert status[i] == 1, (i, name)
        assert after[i][0] == before[i][0] and after[i][2] == before[i][2], (i, name)          # boards and flags stay
        assert after[i][1] == np.float64(value).tobytes(), (i, name, value)
        assert after[i][3] == index.tobytes() and after[i][4] == weight.tobytes(), (i, name)
        assert where[i].tolist() == [at, len(index)], (i, name, where[i], at)                 # appended in call order
        at += len(index)
    assert {"M=1", "M=63", "M=64", "M=65", "M=256", "single", "last round", "ties", "W=nan", "W=inf", "heavy"} <= seen
    assert {names[i] for i in np.flatnonzero(status == 0)} == {"total=0", "finished", "M=0"}
    assert store.counts()["targets"] == at
    called = {tuple(p) for p in pairs.tolist()}
    after_all = snapshot(store)
    assert len(everyone) - len(called) > 50
    for k, p in enumerate(everyone.tolist()):
        if tuple(p) not in called:
            assert after_all[k] == before_all[k], p                                           # plies not in the call
    assert store.mirror()[1].tobytes() == np.array([r[2] for r in after_all], dtype=np.uint8).tobytes()
    # a second call on the same plies appends again, behind the first one's pairs
    status2 = store.retarget(pairs[:70], upload(records[100:170]), 0)
    where2 = store.ply_targets(pairs[:70])
    changed = np.flatnonzero(status2 == 1)
    assert where2[changed[0]][0] == at and store.counts()["targets"] == at + int(where2[changed, 1].sum())
    store.close()


def check_refusals():
    rng = np.random.default_rng(22)
    recs, entries, a = fixture_games()
    # a store with a pass, a BAD ply, a game with "full" and a game on walls
    a.ply_flags[3] |= PASS
    lo, hi = int(a.target_start[70]), int(a.target_start[71])
    a.target_weight[lo:hi] *= F32(0.5)
    a.blockers[10] = np.uint64(1 << 24)
    a.boards[10 * 64:] &= ~np.uint64(1 << 24)
    pairs_all = None
    needed = None
    for attempt in range(2):
        # the second store has room for exactly the targets the good call appends, less one
        spare = PICKED * link.MAX_MOVES if needed is None else needed - 1
        store = link.SampleStore(len(a.games) + 1, len(a.ply_flags) + 64, len(a.target_index) + spare)
        store.add_arrays(a)
        games, flags = store.mirror()
        assert flags[3] & PASS and flags[70] & BAD
        if pairs_all is None:
            good = [p for p in eligible_pairs(store) if p[0] != 10]
            pairs_all = np.array([good[int(k)] for k in rng.choice(len(good), size=PICKED, replace=False)], dtype=np.int32)
            records, _ = ref.shaped_records(rng, PICKED)
            needed = sum(len(ref.retarget(r)[0]) for r in records)
        reports = upload(records)
        not_full = next(p for p in range(64) if not flags[4 * 64 + p] & FULL)
        before, counts = snapshot(store), store.counts()

        def refused(code, pairs, reports=reports, blockers=0):
            try:
                store.retarget(pairs, reports, blockers)
            except link.AzhError as err:
                assert "error %d" % code in str(err), err
            else:
                raise AssertionError("the call was accepted")
            assert snapshot(store) == before and store.counts() == counts

        if attempt == 1:
            refused(-6, pairs_all)                                      # cap_targets one short
            store.close()
            break
        swapped = pairs_all.copy()
        swapped[17] = (0, 3)
        refused(-1, swapped)                                            # a pass
        swapped[17] = (1, 6)
        refused(-2, swapped)                                            # a BAD ply (ply 70 of the store)
        swapped[17] = (4, not_full)
        refused(-1, swapped)                                            # not FULL in a game that has "full"
        swapped[17] = pairs_all[400]
        refused(-1, swapped)                                            # a pair given twice
        swapped[17] = (12, 0)
        refused(-1, swapped)                                            # out of range
        refused(-2, pairs_all, blockers=1 << 24)                        # the reports' walls are not the games'
        wall_pairs = np.array([p for p in eligible_pairs(store) if p[0] == 10][:8], dtype=np.int32)
        refused(-2, wall_pairs)                                         # and the other way round
        for bad in ref.malformed_records(rng):
            broken = records.copy()
            broken[317] = bad
            refused(-2, pairs_all, upload(broken))                      # one malformed record among 600
        # the good call, then a game appended behind the new tail, then a minibatch that reads old and new plies
        status = store.retarget(pairs_all, reports, 0)
        assert store.counts()["targets"] == counts["targets"] + needed
        walled = store.retarget(wall_pairs, upload(records[:8]), 1 << 24)
        tail = store.counts()["targets"]
        extra_rec = random_record(np.random.default_rng(99), 30, 50, kind=16, uid=12)
        extra = link.pack_records(extra_rec)
        store.add_arrays(extra)
        new_pairs = np.array([(12, p) for p in range(30)], dtype=np.int32)
        where = store.ply_targets(new_pairs)
        assert where[0][0] == tail and where[:, 1].tolist() == np.diff(extra.target_start).tolist()
        got = store.read_plies(new_pairs)
        assert got[0].tobytes() == extra.boards.tobytes() and got[4].tobytes() == extra.target_index.tobytes() and \
            got[5].tobytes() == extra.target_weight.tobytes()
        lines = [json.loads(link.format_record_json(r)) for r in recs] + [json.loads(link.format_record_json(extra_rec))]
        lines[10]["blockers"] = link.blockers_to_cells(1 << 24)
        cells = link.blockers_to_cells(1 << 24)
        for board in lines[10]["boards"]:
            for c in cells:
                board[c] = 0
        apply_to_entries(lines, pairs_all, records, status)
        apply_to_entries(lines, wall_pairs, records[:8], walled)
        changed = pairs_all[status == 1]
        draws = [(int(g), int(p), k % 8) for k, (g, p) in enumerate(changed[:40].tolist())] + \
                [(12, p, p % 8) for p in range(30)] + [(int(g), int(p), 3) for g, p in wall_pairs.tolist()] + \
                [(2, p, 5) for p in range(64) if (2, p) not in {tuple(q) for q in pairs_all.tolist()} and
                 not flags[2 * 64 + p] & (PASS | BAD)]
        for blend in (0.0, 0.5):
            same(host(store.gather(draws, blend)), first_three(lines, draws, blend), blend)
        store.close()


def check_minibatch_parity():
    rng = np.random.default_rng(23)
    store, entries, a, pairs, records, names = synthetic_store(PICKED * link.MAX_MOVES, rng)
    status = store.retarget(pairs, upload(records), 0)
    apply_to_entries(entries, pairs, records, status)
    called = {tuple(p) for p in pairs.tolist()}
    changed = [tuple(p) for p in pairs[status == 1].tolist()]
    kept = [tuple(p) for p in pairs[status == 0].tolist()]
    flags = store.mirror()[1]
    outside = [tuple(p) for p in all_pairs(store).tolist() if tuple(p) not in called and not flags[64 * p[0] + p[1]] & BAD]
    # the reply target of the ply before a changed one
    before = [(g, p - 1) for g, p in changed if p > 0 and not flags[64 * g + p - 1] & BAD]
    assert len(kept) > 20 and len(outside) > 20 and len(before) > 100
    picks = changed[:24] + kept[:8] + outside[:8] + before[:24]
    # every shape's ply at least once
    first_of = {}
    for i, name in enumerate(names):
        first_of.setdefault(name, tuple(pairs[i].tolist()))
    picks += list(first_of.values())
    for s in range(8):
        draws = [(g, p, s) for g, p in picks]
        for blend in (0.0, 0.5):
            want = first_three(entries, draws, blend)
            same(host(store.gather(draws, blend)), want, (s, blend))
            got = host(store.gather(draws, blend, aux=True))
            same(got[:3], want, (s, blend, "aux"))
            for k, (g, p, _) in enumerate(draws):                       # the reply: ply p + 1's target as it is now
                e = entries[g]
                present = p + 1 < len(e["boards"]) and ("full" not in e or bool(e["full"][p + 1]))
                heat = ar.heat_map(e, p + 1, s) if present else None
                assert got[6][k, 1] == (0.0 if heat is None else 1.0), (g, p, s)
                assert got[5][k].tobytes() == (np.zeros((7, 7, 17), F32) if heat is None else heat).tobytes(), (g, p, s)
    assert float(np.abs(want[2]).min()) < 0.999                         # the blend moved value targets
    store.close()


def played_games(net, mask, fen, seed):
    """Real games of an 8-slot, 8-visit engine cut at 12 plies -> (record words, the games' lines in record order)."""
    cfg = selfplay.make_config(8, 8, seed=seed, fen=fen, max_plies=12, flags=link.FLAG_KEEP_UNFINISHED)
    assert int(cfg.blockers) == mask
    e = link.Engine(cfg)
    e.set_resign(0.0, 3, 0)                      # the search's values are recorded, nobody resigns
    e.run(net, 260, link.DTYPE_F32)
    e.fetch()
    words = e.staged_records().copy()
    e.close()
    recs = list(link.records(words))
    assert len(recs) >= 8
    lines = [json.loads(link.format_record_json(r.words, blockers=mask if mask else None)) for r in recs]
    return np.concatenate([r.words for r in recs]), lines


def bitboards(entry, ply):
    cells = np.asarray(entry["boards"][ply], dtype=np.int8)
    return tuple(int(((cells == v) * link._CELL_BIT).sum(dtype=np.uint64)) for v in (1, 2))


def whole_path(starts, picks, seed):
    """Games played on each of `starts` = (mask, FEN) go into one store; training.reanalyse searches `picks` of their plies at 8
    slots and 16 visits in f32; a second engine per mask, driven by the calls that were there before, gives the reports the
    store's new targets and values are restated from."""
    conv, bn = model.random_init(2, 64, seed=5, perturb_bn=True)
    net = link.Net(conv, bn)
    store = link.SampleStore(128, 128 * 12, 128 * 12 * 100 + picks * link.MAX_MOVES)
    entries = []
    for k, (mask, fen) in enumerate(starts):
        words, lines = played_games(net, mask, fen, seed + k)
        store.add_records(words, mask, aux=True)
        entries += lines
    games, flags = store.mirror()
    cand, count, _, _ = store.ply_cum()
    masks = store.game_blockers()
    assert sorted(set(int(m) for m in masks)) == sorted(m for m, _ in starts) and store.counts()["bad_plies"] == 0
    c = len(eligible_pairs(store))
    plan = training.reanalyse_plan(games, flags, cand, count, masks, 0, len(games), picks / c, 8, seed=3)
    assert sum(len(rows) for _, rows in plan) == picks
    per_mask = {}
    for mask, rows in plan:
        per_mask.setdefault(mask, []).append(len(rows))
    assert sorted(per_mask) == sorted(m for m, _ in starts)
    for sizes in per_mask.values():                                      # full rounds, then the rest, per mask
        assert all(n == 8 for n in sizes[:-1]) and 0 < sizes[-1] <= 8, per_mask
    if len(starts) == 1:
        assert per_mask == {0: [8, 8, picks - 16]} and 0 < picks - 16 < 8    # three rounds, the last one short
    made, log, make = [], [], link.Engine

    def spy(cfg):
        made.append(int(cfg.blockers))
        return make(cfg)

    link.Engine = spy
    try:
        before = snapshot(store)
        out = training.reanalyse(store, net, link.DTYPE_F32, plan, 16, 8, log.append)
    finally:
        link.Engine = make
    assert made == sorted(per_mask), (made, per_mask)                    # one engine per mask, given that mask
    assert out["changed"] == picks and out["unchanged"] == 0 and out["rounds"] == len(plan), out
    assert len(log) == 1 and ("Reanalysis: %d plies changed, 0 unchanged in %d rounds" % (picks, len(plan))) in log[0]
    assert out["mean_kl"] > 0.0 and np.isfinite(out["mean_kl"])
    # the same searches by existing calls only: boards from the game lines, set_positions, run, the host's root_report
    max_plies = int(games[:, 1].max()) + 1
    all_pairs_, all_records = [], []
    engine, engine_mask = None, None
    for mask, rows in plan:
        if engine is None or engine_mask != mask:
            if engine is not None:
                engine.close()
            engine, engine_mask = link.Engine(training.reanalysis_config(8, 16, mask, max_plies)), mask
        boards = np.zeros((8, 2), dtype=np.uint64)
        plies = np.zeros(8, dtype=np.int32)
        for i in range(8):
            g, p = (int(v) for v in rows[i if i < len(rows) else 0])
            x, o = bitboards(entries[g], p)
            boards[i] = (x | (p & 1) << 63, o)
            plies[i] = p
        engine.set_positions(boards, plies)
        engine.run(net, 17, link.DTYPE_F32)
        words = np.zeros((8, link.ROOT_REPORT_WORDS), dtype=np.uint32)
        link.check(link.load().azh_engine_root_report(engine.h, 0, 8, words.ctypes.data))
        device = torch.zeros(8 * link.ROOT_REPORT_WORDS, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        engine.root_report_device(device, 0, 8)
        assert device.cpu().numpy().view(np.uint32).tobytes() == words.tobytes()          # the same records, left on the device
        for i in range(len(rows)):
            assert int(words[i][5:5 + 4 * int(words[i][1]):4].sum()) == 16 and words[i][3] == 0, (mask, i)
        all_pairs_.append(rows)
        all_records.append(words[:len(rows)])
    engine.close()
    pairs, records = np.concatenate(all_pairs_), np.concatenate(all_records)
    after = snapshot(store, pairs)
    for i, rec in enumerate(records):
        index, weight, value = ref.retarget(rec)
        assert after[i][3] == index.tobytes() and after[i][4] == weight.tobytes(), i
        assert after[i][1] == np.float64(value).tobytes(), i
    called = {tuple(p) for p in pairs.tolist()}
    after_all = snapshot(store)
    for k, p in enumerate(all_pairs(store).tolist()):
        if tuple(p) not in called:
            assert after_all[k] == before[k], p
    # minibatch parity on the lines with the reanalysed plies' dists and values replaced, the seven arrays
    apply_to_entries(entries, pairs, records, np.ones(len(pairs), dtype=np.int32))
    picks_ = [tuple(p) for p in pairs.tolist()] + [(g, p - 1) for g, p in pairs.tolist() if p > 0]
    picks_ += [tuple(p) for p in all_pairs(store).tolist() if tuple(p) not in called][:10]
    for s in range(8):
        draws = [(g, p, s) for g, p in picks_]
        for blend in (0.0, 0.5):
            want = restated(entries, draws, blend)
            same(host(store.gather(draws, blend, aux=True)), want, (s, blend))
            same(host(store.gather(draws, blend)), want[:3], (s, blend))
    # the surprise of the new targets: azh_samples_surprise_host on the new pairs in stored (edge) order
    n_plies = store.counts()["plies"]
    logits = (3.0 * np.random.default_rng(4).standard_normal((n_plies, 833))).astype(F32)
    got, illegal = store.surprise_from_logits(0, torch.from_numpy(logits).cuda())
    assert illegal == 0
    boards, _, _, start, index, weight = store.read_plies(pairs)
    positive = 0
    for i, (g, p) in enumerate(pairs.tolist()):
        mover, opponent = (int(boards[i][p & 1]), int(boards[i][1 - (p & 1)]))
        want, missing = link.samples_surprise_host_blockers(logits[int(games[g][0]) + p], mover, opponent, int(masks[g]),
                                                            index[start[i]:start[i + 1]], weight[start[i]:start[i + 1]])
        assert missing == 0 and np.float32(want).tobytes() == got[int(games[g][0]) + p].tobytes(), (g, p)
        positive += want > 0
    assert positive >= len(pairs) - 2
    net.close()
    store.close()


def check_whole_path():
    whole_path([(0, selfplay.START_FEN_PLAIN)], 20, seed=31)


def check_walls():
    _, _, mask, _ = selfplay.parse_fen(selfplay.START_FEN_SELFPLAY)
    assert mask
    whole_path([(0, selfplay.START_FEN_PLAIN), (mask, selfplay.START_FEN_SELFPLAY)], 23, seed=41)


CHECKS = [check_read_plies, check_synthetic_reports, check_refusals, check_minibatch_parity, check_whole_path, check_walls]


if __name__ == "__main__":
    fresh_process.main(CHECKS)
