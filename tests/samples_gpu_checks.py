"""The device checks of tests/test_gpu_samples.py, run in a process of their own: a SampleStore writes torch's tensors on
torch's streams, so torch must be imported before the library is loaded (link.require_torch_runtime) — in a pytest process
that has run other device tests it is the other way round.  `python -m tests.samples_gpu_checks OUT.json` runs every check
and writes {name: "ok" | traceback}; after a check that ends in a device error nothing more is run (tests/fresh_process.py).
What the store's checks modules share is in tests/store_checks.py."""
import ctypes
import json
import random

import numpy as np
import torch

from ataxxzero_amd import link, model, training
from tests import aux_fixtures, fresh_process
from tests.samples_fixtures import MOVES
from tests.store_checks import first_three, golden_entries, host, move_text, same, store_of_entries

F32 = np.float32
BOARD = [(c * 7 + c // 5) % 3 for c in range(49)]            # no symmetry maps it onto itself
MOVE_TEXT = [move_text(a | b << 8) for a, b in MOVES]


def synthetic_entries(seed=1, games=12):
    """Entries of every flavour: "full" (game 1 without one full ply), "values", pass plies with "pass" keys, list-typed moves
    without dists, random_ply."""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(games):
        plies = 1 if g == 5 else int(rng.integers(3, 24))
        boards = [[int(v) for v in rng.integers(0, 3, size=49)] for _ in range(plies)]
        e = {"boards": boards, "result": 1 + g % 2}
        if g % 4 == 3:                                        # the Python generator's entries: one-hot on the move played
            e["moves"] = []
            for p in range(plies):
                a, b = MOVES[int(rng.integers(len(MOVES)))]
                to = [b % 7, 6 - b // 7]
                e["moves"].append(["c", to] if a == b else [[a % 7, 6 - a // 7], to])
            out.append(e)
            continue
        e["moves"], e["dists"] = [], []
        for p in range(plies):
            if plies > 2 and p % 7 == 4:
                e["moves"].append("pass")
                e["dists"].append({"pass": 1.0})
                continue
            k = int(rng.integers(1, 30))
            chosen = [MOVE_TEXT[j] for j in rng.choice(len(MOVE_TEXT), size=k, replace=False)]
            counts = rng.integers(1, 400, size=k)
            e["moves"].append(chosen[0])
            e["dists"].append({m: float(c) / float(counts.sum()) for m, c in sorted(zip(chosen, counts))})
        if g % 3 == 1:
            e["full"] = [0] * plies if g == 1 else [int(v) for v in rng.integers(0, 2, size=plies)]
            if g != 1:
                e["full"][0] = 1
        if g % 2 == 0:
            e["values"] = [float(v) for v in rng.uniform(-1, 1, size=plies)]
        if g % 6 == 2 and plies > 2:
            e["random_ply"] = int(rng.integers(0, plies - 1))
        out.append(e)
    return out


# ---------------------------------------------------------------- the checks

def check_reference_parity():
    entries = golden_entries() + synthetic_entries()
    assert any("random_ply" in e for e in entries) and any("dists" not in e for e in entries)
    store = store_of_entries(entries)
    c = store.counts()
    assert c["games"] == len(entries) and c["plies"] == sum(len(e["boards"]) for e in entries)
    for blend in (0.0, 0.5):
        for seed in range(4):
            random.seed(seed)
            want = training.make_minibatch_reference(entries, 200, blend)
            state = random.getstate()
            random.seed(seed)
            got = host(training.make_minibatch_device(store, 0, len(entries), 200, blend))
            assert random.getstate() == state
            same(got, want)
    assert np.abs(want[2]).min() < 0.999            # the blend moved some value targets
    # a sub-range is entries[first:first + n]
    random.seed(9)
    want = training.make_minibatch_reference(entries[5:17], 64, 0.5)
    random.seed(9)
    same(host(training.make_minibatch_device(store, 5, 12, 64, 0.5)), want)
    store.close()


def check_every_index_under_every_symmetry():
    assert len(MOVE_TEXT) == len(set(MOVE_TEXT)) == 529
    entry = {"boards": [BOARD] * 529, "moves": MOVE_TEXT, "result": 2}
    store = store_of_entries([entry])
    seen = set()
    for s in range(8):
        feats, pols, vals = host(store.gather([(0, p, s) for p in range(529)]))
        for p, text in enumerate(MOVE_TEXT):
            heat = np.zeros((7, 7, 17), dtype=F32)
            training.add_move_to_heatmap(heat, training.apply_symmetry_to_move(s, training.uai_decode_move(text)))
            assert pols[p].tobytes() == heat.tobytes(), (s, text)
            want = training.apply_symmetry(s, training.board_to_features(BOARD, 1 + p % 2)).astype(F32)
            assert feats[p].tobytes() == want.tobytes(), (s, p)
            assert vals[p, 0] == (1 if 1 + p % 2 == 2 else -1)
        seen.add(feats[0].tobytes())
    assert len(seen) == 8                           # the board is asymmetric: eight different images
    store.close()


def check_edges_of_the_wave():
    rng = np.random.default_rng(3)
    entries = []
    for k in (1, 63, 64, 65, 128, 529):
        chosen = [MOVE_TEXT[j] for j in rng.choice(529, size=k, replace=False)]
        w = rng.dirichlet(np.ones(k))
        entries.append({"boards": [[int(v) for v in rng.integers(0, 3, size=49)]], "moves": [chosen[0]], "result": 1,
                        "dists": [{m: float(x) for m, x in zip(chosen, w)}]})
    store = store_of_entries(entries)
    assert store.counts()["bad_plies"] == 0 and store.counts()["targets"] == 1 + 63 + 64 + 65 + 128 + 529
    for size in (1, 63, 64, 65, 257):
        random.seed(size)
        want = training.make_minibatch_reference(entries, size)
        random.seed(size)
        same(host(training.make_minibatch_device(store, 0, len(entries), size)), want)
    store.close()


def check_the_record_path():
    from tests.engine_harness import START
    conv, bn = model.random_init(1, 128, seed=3, perturb_bn=True)
    net = link.Net(conv, bn)
    x, o, turn = START
    kinds = set()
    for gumbel in (False, True):
        cfg = link.Config(games=8, visits=16, max_plies=400, edges_per_node=96, c_puct=1.0, dirichlet_alpha=0.15,
                          dirichlet_weight=0.0 if gumbel else 0.25, start_turn=turn, seed=77, start_x=x, start_o=o, blockers=0,
                          flags=link.FLAG_NO_REUSE if gumbel else 0)
        e = link.Engine(cfg)
        if gumbel:
            e.set_gumbel(4, 50.0, 1.0)
        else:
            e.set_playout_cap(6, 32768)
            e.set_resign(0.0, 3, 0)              # values recorded, nobody resigns
        e.run(net, 1200, link.DTYPE_BF16)
        e.fetch()
        words = e.staged_records().copy()
        lines = e.drain_json()
        e.close()
        recs = list(link.records(words))         # (without the markers of dropped games)
        assert len(recs) == len(lines) >= 4
        kinds |= {r.kind for r in recs}
        recs.sort(key=lambda r: r.uid)           # the lines come in uid order
        entries = [json.loads(line) for line in lines]
        assert [len(en["boards"]) for en in entries] == [len(r.plies) for r in recs]
        store = link.SampleStore(len(recs), sum(len(r.plies) for r in recs), len(words))
        store.add_records(np.concatenate([r.words for r in recs]))
        for blend in (0.0, 0.5):
            random.seed(5)
            want = training.make_minibatch_reference(entries, 128, blend)
            random.seed(5)
            same(host(training.make_minibatch_device(store, 0, len(entries), 128, blend)), want)
        store.close()
    assert any(k & link.REC_KIND_GUMBEL for k in kinds) and \
        any(k & link.REC_KIND_VALUES and k & link.REC_KIND_PLAYOUT_CAP for k in kinds)
    net.close()


def drawable_mix():
    """40 games, the first 10 and half of the rest without a drawable ply."""
    entries = synthetic_entries(seed=2, games=40)
    for g, e in enumerate(entries):
        if g < 10 or g % 2:
            plies = len(e["boards"])
            if g % 3 == 0 and "dists" in e:
                e["dists"] = [{k: v * 0.5 for k, v in d.items()} for d in e["dists"]]     # every target sums to a half
            else:
                e.pop("random_ply", None)
                e["full"] = [0] * plies                                                   # "full" without a full ply
    return entries


def check_device_draws():
    entries = drawable_mix()
    store = store_of_entries(entries)
    games, flags = store.mirror()
    assert store.counts()["bad_plies"] > 0
    n, first, count = 257, 10, len(entries) - 10
    draws_out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    for step in range(3):
        out = host(store.draw_gather(n, 99, step, first, count, 0.5, draws_out=draws_out))
        draws = draws_out.cpu().numpy()
        for i in range(n):
            assert tuple(int(v) for v in draws[i]) == store.draw(99, step, i, first, count), (step, i)
            g, ply, s, attempts = (int(v) for v in draws[i])
            assert first <= g < len(entries) and 1 <= attempts <= 64 and 0 <= s < 8 and 0 <= ply < games[g][1]
            f = int(flags[int(games[g][0]) + ply])
            assert not f & (link.SAMPLES_PLY_PASS | link.SAMPLES_PLY_BAD)
            assert games[g][3] == ply if games[g][3] else (f & link.SAMPLES_PLY_FULL or not games[g][2] & link.SAMPLES_GAME_HAS_FULL)
        same(out, host(store.gather(draws[:, :3], 0.5)))
        same(out, first_three(entries, draws[:, :3].tolist(), 0.5))
    assert store.status() == 0
    # a range of undrawable games only: zeros, counted, and the call ends
    out = store.outputs(n)
    for t in out:
        t.fill_(7.0)
    store.draw_gather(n, 99, 0, 0, 10, 0.0, out=out, draws_out=draws_out)
    assert store.status() == n
    assert all(float(t.abs().max()) == 0.0 for t in out)
    assert (draws_out.cpu().numpy() == np.array([-1, -1, -1, 64])).all()
    store.close()


def check_stream_and_reuse():
    entries = golden_entries() + synthetic_entries()
    store = store_of_entries(entries)
    rng = np.random.default_rng(8)

    def some_draws(n):
        rows = []
        while len(rows) < n:
            g = int(rng.integers(len(entries)))
            ply = int(rng.integers(len(entries[g]["boards"])))
            if entries[g]["moves"][ply] != "pass":
                rows.append((g, ply, int(rng.integers(8))))
        return rows

    a, b = some_draws(300), some_draws(300)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                  # torch's current stream, not the default one
        out_a, out_b = store.outputs(300), store.outputs(300)
        store.gather(a, 0.5, out=out_a)
        store.gather(b, 0.5, out=out_b)            # back to back: the other staging buffer
        sums = [t.sum(dim=tuple(range(1, t.dim()))) for t in out_a + out_b]      # consumed with no host wait in between
        doubled = out_b[1] * 2
    side.synchronize()
    want_a, want_b = first_three(entries, a, 0.5), first_three(entries, b, 0.5)
    same(host(out_a), want_a)
    same(host(out_b), want_b)
    assert doubled.cpu().numpy().tobytes() == (want_b[1] * 2).tobytes()
    for got, want in zip(sums, want_a + want_b):
        assert np.allclose(got.cpu().numpy(), want.reshape(300, -1).sum(axis=1), atol=1e-4)
    # torch's default stream (the null stream): a gather into tensors that work enqueued earlier still reads must wait for it
    out = store.outputs(300)
    store.gather(a, 0.5, out=out)
    big = torch.ones((4096, 4096), device="cuda")
    for _ in range(20):                            # some milliseconds of work in front of the reader
        big = (big @ big) * (1.0 / 4096)
    kept = out[1] + (big[0, 0] - 1.0)              # reads the first minibatch once that work is done
    store.gather(b, 0.5, out=out)                  # enqueued right away, into the same tensors
    assert kept.cpu().numpy().tobytes() == want_a[1].tobytes()
    same(host(out), want_b)
    store.close()


def check_capacity():
    entries = synthetic_entries(seed=4, games=6)
    a = link.entries_to_arrays(entries)
    extra = link.entries_to_arrays(synthetic_entries(seed=6, games=1))
    draws = [(g, 0, g % 8) for g in range(6)]
    for spare in ((0, 99, 9999), (9, 0, 9999), (9, 99, 0)):
        store = link.SampleStore(len(a.games) + spare[0], len(a.ply_flags) + spare[1], len(a.target_index) + spare[2])
        store.add_arrays(a)
        counts = store.counts()
        before = host(store.gather(draws, 0.5))
        try:
            store.add_arrays(extra)
        except link.AzhError as err:
            assert "error -6" in str(err), err
        else:
            raise AssertionError("one game beyond the capacity was accepted")
        assert store.counts() == counts
        same(host(store.gather(draws, 0.5)), before)
        store.close()


def check_bad_ply():
    entries = synthetic_entries(seed=4, games=3)
    bad = {"boards": [BOARD], "moves": ["a1"], "result": 1, "dists": [{"a1": 0.25, "b2": 0.25}]}
    store = store_of_entries(entries + [bad])
    assert store.counts()["bad_plies"] == 1
    for fn in (lambda: training.make_minibatch_reference([bad], 4), lambda: training.make_minibatch([bad], 4),
               lambda: training.make_minibatch_device(store, 3, 1, 4)):
        random.seed(1)
        try:
            fn()
        except AssertionError as err:
            assert str(err) == "policy target does not sum to one"
        else:
            raise AssertionError("a bad ply was accepted")
    out = store.outputs(2)
    for t in out:
        t.fill_(7.0)
    try:
        store.gather([(0, 0, 0), (3, 0, 1)], out=out)
    except AssertionError as err:
        assert str(err) == "policy target does not sum to one"
    else:
        raise AssertionError("a bad ply was accepted")
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in out)          # nothing was launched
    for draw in ((4, 0, 0), (0, 999, 0), (0, 0, 8), (-1, 0, 0)):
        try:
            store.gather([draw], out=store.outputs(1))
        except link.AzhError:
            pass
        else:
            raise AssertionError("draw %r was accepted" % (draw,))
    store.close()


def check_argument_refusals():
    """One to three of the four auxiliary outputs: -1, nothing launched, and the calls that follow are a fresh store's; a target
    count that is not where target_start ends: -2, nothing added."""
    arrays = link.entries_to_arrays([aux_fixtures.cut(aux_fixtures.walled_games()[0][0], 2)], aux=True)
    assert len(arrays.games) == 1 and len(arrays.ply_flags) == 2 and 2 <= len(arrays.target_index) <= 24
    fresh, store = link.SampleStore(2, 4, 48), link.SampleStore(2, 4, 48)
    fresh.add_arrays(arrays)
    store.add_arrays(arrays)
    draws = np.array([[0, 0, 5]], dtype=np.int32)
    want = [host(fresh.gather(draws)), host(fresh.gather(draws, aux=True)), host(fresh.draw_gather(1, 9, 0, 0, 1)),
            host(fresh.draw_gather(1, 9, 0, 0, 1, aux=True))]
    assert want[1][6].tolist() == [[0.0, 1.0]] and want[1][5].any() and want[0][1].any()     # (cut short: no owners; a reply)
    out = store.aux_outputs(1)
    for t in out:
        t.fill_(7.0)
    whole, stream = store._pointers(out, 1)
    lib = link.load()
    for given in ((3,), (4,), (5,), (6,), (3, 4), (4, 6), (3, 4, 5), (4, 5, 6)):
        part = link.CSampleOutputs(*[getattr(whole, name) if k < 3 or k in given else None
                                     for k, (name, _) in enumerate(link.CSampleOutputs._fields_)])
        assert lib.azh_samples_gather(store.h, 1, draws.ctypes.data, 0.0, ctypes.byref(part), stream) == -1, given
        assert lib.azh_samples_draw_gather(store.h, 1, 9, 0, 0, 1, 0.0, ctypes.byref(part), None, stream) == -1, given
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in out) and store.status() == 0      # nothing was launched
    got = [host(store.gather(draws)), host(store.gather(draws, aux=True)), host(store.draw_gather(1, 9, 0, 0, 1)),
           host(store.draw_gather(1, 9, 0, 0, 1, aux=True))]
    for g, w in zip(got, want):
        assert len(g) == len(w) and all(x.tobytes() == y.tobytes() for x, y in zip(g, w))
    counts = store.counts()
    for off in (-1, 1):
        c = arrays.c_arrays()
        c.n_targets += off
        assert lib.azh_samples_add_games(store.h, ctypes.byref(c)) == -2, off
        assert store.counts() == counts
    store.add_arrays(arrays)                                 # and the arrays as they are go in
    assert store.counts()["games"] == 2
    fresh.close()
    store.close()


CHECKS = [check_reference_parity, check_every_index_under_every_symmetry, check_edges_of_the_wave, check_the_record_path,
          check_device_draws, check_stream_and_reuse, check_capacity, check_bad_ply, check_argument_refusals]


if __name__ == "__main__":
    fresh_process.main(CHECKS)
