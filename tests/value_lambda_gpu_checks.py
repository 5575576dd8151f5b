"""The device checks of tests/test_gpu_value_lambda.py, run in a process of their own (as tests/prove_gpu_checks.py, and for its
reason: a SampleStore needs torch imported before the library is loaded).  `python -m tests.value_lambda_gpu_checks OUT.json`
runs every check and writes {name: "ok" | traceback}; after a check that ends in a device error nothing more is run.

The store: slices of the six golden games, cut so that x moves on their even plies, of 1, 2, 63, 64, 65, 128 and 129 plies
— the chunk edges of a 64-lane walk — and others, one game of 300 plies, and one game without values.  Most slices end where
their game ended, where a depth-2 search proves plies."""
import random

import numpy as np
import torch

from ataxxzero_amd import link, training
from tests import fresh_process, store_checks
from tests import lambda_reference as lr
from tests.store_checks import all_pairs, host, same, store_of_entries

LENGTHS = (1, 2, 63, 64, 65, 128, 129, 3, 17, 100, 130, 200)
LONG = 300
NO_VALUES = 9                      # the game that carries no values
_cache = {}


def piece(entry, start, n):
    """plies [start, start + n) of a game line as a game line of its own; start is even: x still moves on the even plies"""
    assert start % 2 == 0 and 0 <= start and start + n <= len(entry["boards"])
    out = {"boards": entry["boards"][start:start + n], "moves": entry["moves"][start:start + n], "result": entry["result"]}
    if "dists" in entry:
        out["dists"] = entry["dists"][start:start + n]
    return out


def entries():
    if "entries" not in _cache:
        golden = store_checks.golden_entries()
        rng = np.random.default_rng(7)
        made = []
        for k in range(2 * len(LENGTHS)):
            e, n = golden[k % len(golden)], LENGTHS[k % len(LENGTHS)]
            T = len(e["boards"])
            made.append(piece(e, (T - n) // 2 * 2, n))                       # the game's end, or one ply short of it
        long_game = piece(golden[5], 0, 260)
        tail = piece(golden[0], 0, LONG - 260)
        for key in ("boards", "moves", "dists"):
            long_game[key] = long_game[key] + tail[key]
        made.insert(5, long_game)
        for g, e in enumerate(made):
            if g != NO_VALUES:
                e["values"] = rng.uniform(-1.0, 1.0, len(e["boards"])).tolist()
        assert sorted(set(len(e["boards"]) for e in made)) == sorted(set(LENGTHS + (LONG,))) and len(made) == 25
        _cache["entries"] = made
    return _cache["entries"]


def fresh_store():
    store = store_of_entries(entries())
    assert store.counts()["bad_plies"] == 0 and store.counts()["games"] == len(entries())
    return store


def restated(lam, proofs=None):
    """{game: [G_p]} of every game with values, from tests/lambda_reference.py; proofs: one word per (game, ply) of all_pairs"""
    key = (lam, None if proofs is None else tuple(int(v) for v in proofs))
    if key not in _cache:
        out, at = {}, 0
        for g, e in enumerate(entries()):
            n = len(e["boards"])
            if "values" in e:
                out[g] = lr.returns(e["values"], e["result"], lam, None if proofs is None else proofs[at:at + n])
            at += n
        _cache[key] = out
    return _cache[key]


def expect_returns(store, want, what):
    """want: {game: [G_p]} the covered games; every other ply must read absent"""
    pairs = all_pairs(store)
    got, present = store.read_value_returns(pairs)
    covered = np.array([g in want for g, _ in pairs.tolist()])
    assert present.tolist() == covered.tolist(), what
    assert not got[~covered].any(), what
    flat = [want[g][p] for g, p in pairs.tolist() if g in want]
    assert lr.bits(got[covered]) == lr.bits(flat), what


def within(want, first, n):
    return {g: G for g, G in want.items() if first <= g < first + n}


def chosen_draws(store):
    """Every ply of the games of up to 65 plies, and the chunk edges, the ends and every fifth ply of the longer ones"""
    games, _ = store.mirror()
    picks = []
    for g in range(len(games)):
        T = int(games[g][1])
        picks += [(g, p) for p in range(T) if T <= 65 or p % 5 == 0 or p < 2 or p >= T - 3 or (T - p) % 64 in (0, 1, 63)]
    return np.array([(g, p, k % 8) for k, (g, p) in enumerate(picks)], dtype=np.int32)


def batches(store, draws, seed=99, blends=(0.0, 0.5)):
    """gather and draw_gather, without and with the auxiliary outputs, per value_blend -> {name: arrays}; a draw_gather's draws
    ride along as its last array"""
    out = {}
    n_games = store.counts()["games"]
    for blend in blends:
        for aux in (False, True):
            out["gather", blend, aux] = host(store.gather(draws, blend, aux=aux))
            drawn = torch.zeros((len(draws), 4), dtype=torch.int32, device="cuda")
            got = store.draw_gather(len(draws), seed, 3, 0, n_games, blend, draws_out=drawn, aux=aux)
            out["draw_gather", blend, aux] = host(got) + (drawn.cpu().numpy(),)
    assert store.status() == 0
    return out


def identical(before, after, what):
    assert before.keys() == after.keys()
    for key in before:
        for k, (b, a) in enumerate(zip(before[key], after[key])):
            assert a.tobytes() == b.tobytes(), (what, key, k)


def compare_batches(before, after, draws, want):
    """Everything but the value column byte-identical (the draws included); the value of a sample on a covered ply is (float)G_p,
    every other value what it was -> the covered samples met"""
    met = 0
    for key in before:
        b, a = before[key], after[key]
        rows = np.asarray(draws)[:, :3] if key[0] == "gather" else a[-1][:, :3]
        for t in range(len(b)):
            if t != 2:
                assert a[t].tobytes() == b[t].tobytes(), (key, t)
        value = b[2].copy()
        for k, (g, p, _) in enumerate(rows.tolist()):
            if g in want:
                value[k, 0] = lr.as_f32([want[g][p]])[0]
                met += 1
        assert a[2].dtype == np.float32 and a[2].tobytes() == value.tobytes(), key
    return met


# ---------------------------------------------------------------- the checks

def check_returns_are_the_restatement():
    store = fresh_store()
    G = len(entries())
    expect_returns(store, {}, "before the first pass")
    for lam in lr.LAMBDAS:
        store.value_returns(1, G - 2, lam)                                   # games 0 and G - 1 stay outside
        want = within(restated(lam), 1, G - 2)
        assert len(want) == G - 3 and NO_VALUES not in want
        expect_returns(store, want, lam)
    store.close()


def check_returns_with_proofs():
    store = fresh_store()
    G = len(entries())
    pairs = all_pairs(store)
    stats = store.prove(0, G, 2)
    proofs = store.proofs(pairs)[0]
    assert stats["wins"] > 10 and stats["losses"] > 0 and stats["contradicted"] > 0
    inside = np.array([1 <= g < G - 1 and g != NO_VALUES for g, _ in pairs.tolist()])
    first = np.array([p == 0 for _, p in pairs.tolist()])
    assert (proofs[inside] != 0).sum() > 10 and ((proofs != 0) & inside & ~first).any()
    for lam in (0.7, 0.5, 1.0):
        store.value_returns(1, G - 2, lam)
        want = within(restated(lam, proofs), 1, G - 2)
        expect_returns(store, want, ("proofs", lam))
        assert lam == 1.0 or want != within(restated(lam), 1, G - 2)         # the proofs had a say
    got, _ = store.read_value_returns(pairs)
    proven = (proofs != 0) & inside
    assert got[proven].tolist() == np.where(proofs[proven] > 0, 1.0, -1.0).tolist()
    # a proven ply trains on +-1 with or without the pass, a covered one on its return
    draws = chosen_draws(store)
    value = host(store.gather(draws))[2]
    want = within(restated(1.0, proofs), 1, G - 2)
    at = {tuple(p): k for k, p in enumerate(pairs.tolist())}
    for k, (g, p, _) in enumerate(draws.tolist()):
        if proofs[at[g, p]]:
            assert value[k, 0] == (1.0 if proofs[at[g, p]] > 0 else -1.0), (g, p)
        elif g in want:
            assert value[k].tobytes() == lr.as_f32([want[g][p]]).tobytes(), (g, p)
    # a deeper proof pass afterwards leaves the returns as they were (stale) until the pass runs again
    more = store.prove(0, G, 3)
    assert more["wins"] + more["losses"] > 0
    expect_returns(store, within(restated(1.0, proofs), 1, G - 2), "stale")
    deeper = store.proofs(pairs)[0]
    store.value_returns(1, G - 2, 0.7)
    expect_returns(store, within(restated(0.7, deeper), 1, G - 2), "recomputed")
    store.close()


def check_minibatches_write_the_returns():
    store = fresh_store()
    G = len(entries())
    draws = chosen_draws(store)
    before = batches(store, draws)
    store.value_returns(1, G - 2, 0.7)
    want = within(restated(0.7), 1, G - 2)
    after = batches(store, draws)
    met = compare_batches(before, after, draws, want)
    assert met > 8 * 400, met
    outside = sum(1 for g, _, _ in draws.tolist() if g not in want)
    assert outside > 60                                                      # games 0, G - 1 and the one without values
    drawn = before["draw_gather", 0.0, False][-1][:, 0]
    assert set(drawn.tolist()) >= {0, NO_VALUES, G - 1, 5}                   # the device's own draws met every kind of game
    store.close()


def check_lambda_one_and_zero():
    store = fresh_store()
    G = len(entries())
    draws = chosen_draws(store)
    before = batches(store, draws, blends=(0.0, 1.0))
    store.value_returns(0, G, 1.0)
    ones = batches(store, draws, blends=(0.0,))
    store.value_returns(0, G, 0.0)
    zeros = batches(store, draws, blends=(0.0,))
    for kind in ("gather", "draw_gather"):
        for aux in (False, True):
            for k, b in enumerate(before[kind, 0.0, aux]):
                assert ones[kind, 0.0, aux][k].tobytes() == b.tobytes(), (kind, aux, k)         # lambda 1: z, today's bytes
            for k, b in enumerate(before[kind, 1.0, aux]):
                assert zeros[kind, 0.0, aux][k].tobytes() == b.tobytes(), (kind, aux, k)        # lambda 0: value_blend = 1.0
    assert before["gather", 0.0, False][2].tobytes() != before["gather", 1.0, False][2].tobytes()
    store.close()


def check_clear_restores_every_byte():
    store = fresh_store()
    G = len(entries())
    draws = chosen_draws(store)
    before = batches(store, draws)
    store.clear_value_returns()                                              # nothing to clear: nothing happens
    store.value_returns(0, G, 0.5)
    assert batches(store, draws)["gather", 0.0, False][2].tobytes() != before["gather", 0.0, False][2].tobytes()
    store.clear_value_returns()
    expect_returns(store, {}, "cleared")
    identical(before, batches(store, draws), "cleared")
    store.value_returns(3, 2, 0.9)                                           # and the array comes back empty
    expect_returns(store, within(restated(0.9), 3, 2), "after a clear")
    store.close()


def check_second_pass_and_sub_range():
    store = fresh_store()
    G = len(entries())
    store.value_returns(0, G, 0.5)
    expect_returns(store, restated(0.5), "first")
    store.value_returns(0, G, 0.9)                                           # a second pass replaces the first
    expect_returns(store, restated(0.9), "second")
    store.value_returns(4, 8, 0.5)                                           # games [4, 12): the long one and the one without values
    want = dict(restated(0.9))
    want.update(within(restated(0.5), 4, 8))
    assert 5 in within(restated(0.5), 4, 8) and NO_VALUES not in want
    expect_returns(store, want, "sub-range")
    store.close()


def check_refusals_change_nothing():
    G = len(entries())
    for prepared in (False, True):
        store = fresh_store()
        want = {}
        if prepared:
            store.value_returns(2, 6, 0.5)
            want = within(restated(0.5), 2, 6)
        draws = chosen_draws(store)
        before = batches(store, draws)

        def refused(code, *args):
            try:
                store.value_returns(*args)
            except link.AzhError as err:
                assert "error %d" % code in str(err), err
            else:
                raise AssertionError("the call was accepted: %r" % (args,))
            expect_returns(store, want, args)
            identical(before, batches(store, draws), args)

        refused(-2, 0, G, float("nan"))
        refused(-2, 0, G, -0.1)
        refused(-2, 0, G, 1.1)
        refused(-1, 0, G + 1, 0.5)
        refused(-1, G - 1, 2, 0.5)
        refused(-1, -1, 2, 0.5)
        refused(-1, 0, 0, 0.5)
        refused(-1, 0, G + 1, float("nan"))                                  # the range is looked at first
        store.close()


def check_host_and_device_pipelines_agree():
    store = store_checks.store_of(link.entries_to_arrays(entries(), aux=True))   # with the owners the host pipeline finds
    G = len(entries())
    first, n, size, lam = 2, G - 3, 256, 0.7
    store.value_returns(first, n, lam)
    for aux in (False, True):
        random.seed(31)
        want = training.make_minibatch(entries()[first:first + n], size, aux=aux, value_lambda=lam)
        state = random.getstate()
        random.seed(31)
        got = host(training.make_minibatch_device(store, first, n, size, aux=aux))
        assert random.getstate() == state
        same(got, want, ("value_lambda", aux))
    random.seed(31)
    plain = training.make_minibatch(entries()[first:first + n], size)
    assert plain[2].tobytes() != want[2].tobytes() and plain[1].tobytes() == want[1].tobytes()
    store.close()


CHECKS = [check_returns_are_the_restatement, check_returns_with_proofs, check_minibatches_write_the_returns,
          check_lambda_one_and_zero, check_clear_restores_every_byte, check_second_pass_and_sub_range,
          check_refusals_change_nothing, check_host_and_device_pipelines_agree]


if __name__ == "__main__":
    fresh_process.main(CHECKS)
