"""The device checks of tests/test_gpu_prove.py, run in a process of their own (as tests/reanalyse_gpu_checks.py, and for its
reason: a SampleStore needs torch imported before the library is loaded).  `python -m tests.prove_gpu_checks OUT.json` runs
every check and writes {name: "ok" | traceback}; after a check that ends in a device error nothing more is run."""
import numpy as np
import torch

from ataxxzero_amd import link
from tests import alphabeta_cases as ac
from tests import alphabeta_reference as ab
from tests import fresh_process, store_checks
from tests import rules_reference as rr
from tests.reanalyse_reference import policy_index
from tests.store_checks import all_pairs, eligible_pairs, host, store_of

WIN, NO_MOVE = link.ALPHABETA_WIN, 0xFFFF
LAST = 13               # the plies of each golden game the restatement is run on
# proven wins, proven losses and proofs against the mover's z among the last 13 plies of the six golden games, per depth: what
# tests/alphabeta_reference.py yields there
TABLE = {1: (11, 0, 4), 2: (11, 4, 6), 3: (22, 4, 14)}
_cache = {}


def golden_entries():
    entries = store_checks.golden_entries()
    rng = np.random.default_rng(11)
    for e in entries[::2]:                          # every other game carries the search's values: value_blend has a say
        e["values"] = rng.uniform(-1.0, 1.0, len(e["boards"])).tolist()
    return entries


def golden_store(spare_targets=0, room=0):
    store = store_of(link.entries_to_arrays(golden_entries()), (room, 300 * room, spare_targets))
    assert store.counts()["bad_plies"] == 0 and store.counts()["games"] == 6
    return store


def positions(store, pairs):
    """The stored plies as alphabeta_search takes them -> (packed boards (n, 2), one wall mask per board)"""
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    boards = store.read_plies(pairs, targets=False)[0].copy()
    boards[:, 0] |= (pairs[:, 1].astype(np.uint64) & np.uint64(1)) << np.uint64(63)
    return boards, store.game_blockers()[pairs[:, 0]]


def searched(store, pairs, depth, budget=0):
    packed, walls = positions(store, pairs)
    return link.alphabeta_search(packed, walls, depth, budget)


def recount(store, pairs, out, policy):
    """azh_samples_prove's counts from the searches `out` of the eligible plies `pairs`"""
    games, _ = store.mirror()
    values = out.values.astype(np.int64)
    proven = np.abs(values) >= WIN
    z_plus = np.array([(int(games[g][2]) & 0xFF) == 1 + (p & 1) for g, p in pairs], dtype=bool)
    wins = proven & (values > 0)
    return {"visited": len(pairs), "wins": int(wins.sum()), "losses": int((proven & (values < 0)).sum()),
            "contradicted": int((proven & ((values > 0) != z_plus)).sum()),
            "retargeted": int((wins & (out.moves != NO_MOVE)).sum()) if policy else 0, "nodes": int(out.nodes.sum())}


def same_as_search(store, pairs, out, what):
    proof, move, done = store.proofs(pairs)
    want = np.where(np.abs(out.values) >= WIN, out.values, 0)
    assert proof.tolist() == want.tolist(), what
    assert move.tolist() == out.moves.tolist() and done.tolist() == out.depth_done.tolist(), what


def restated_tail():
    """[(game, ply, ab.all_depths(position, 3))] of the last 13 plies of every golden game, computed once"""
    if "tail" not in _cache:
        store = golden_store()
        games, _ = store.mirror()
        pairs = np.array([(g, p) for g in range(6) for p in range(int(games[g][1]) - LAST, int(games[g][1]))], dtype=np.int32)
        boards = store.read_plies(pairs, targets=False)[0]
        store.close()
        _cache["tail"] = [(int(g), int(p), ab.all_depths(rr.Board.from_masks(int(x), int(o), 0, int(p) & 1), 3))
                          for (g, p), (x, o) in zip(pairs.tolist(), boards.tolist())]
    return _cache["tail"]


# ---------------------------------------------------------------- the checks

def check_proofs_are_the_searchs():
    tail = restated_tail()
    for depth in (1, 2, 3):
        store = golden_store()
        pairs = eligible_pairs(store)
        assert len(pairs) == store.counts()["plies"] == 1351          # no pass, no BAD ply, no "full": every ply
        assert store.proofs(pairs)[0].tolist() == [0] * len(pairs) and set(store.proofs(pairs)[1].tolist()) == {NO_MOVE}
        out = searched(store, pairs, depth)
        stats = store.prove(0, 6, depth)
        assert (out.depth_done == depth).all()
        same_as_search(store, pairs, out, depth)
        assert stats == recount(store, pairs, out, False), (depth, stats)
        assert stats["nodes"] == int(out.nodes.sum()) > 0 and stats["contradicted"] > 0
        # the restatement on the last 13 plies of each game, and the counts it yields there
        where = {tuple(p): k for k, p in enumerate(pairs)}
        proof, move, done = store.proofs(pairs)
        wins = losses = against = 0
        games, _ = store.mirror()
        for g, p, per_depth in tail:
            k = where[(g, p)]
            want_move, want_value, _ = per_depth[depth - 1]
            assert (int(move[k]), int(out.values[k]), int(done[k])) == (want_move, want_value, depth), (depth, g, p)
            assert int(proof[k]) == (want_value if abs(want_value) >= WIN else 0), (depth, g, p)
            if proof[k]:
                wins += proof[k] > 0
                losses += proof[k] < 0
                against += (proof[k] > 0) != ((int(games[g][2]) & 0xFF) == 1 + (p & 1))
        assert (wins, losses, against) == TABLE[depth], (depth, wins, losses, against)
        store.close()


def deep_entries():
    """The walled roots of the deep fixture as plies of synthetic games, one game per wall mask: x to move on the even plies, o
    on the odd ones; a side that runs out of roots repeats its own -> (entries, [[the Deep root of every ply] per game])"""
    by_mask = {}
    for r in ac.deep():
        by_mask.setdefault(r.board.masks()[2], ([], []))[r.board.turn].append(r)
    entries, roots = [], []
    for mask, (xs, os_) in sorted(by_mask.items()):
        assert mask and xs and os_, mask
        n = max(len(xs), len(os_))
        line = [(xs, os_)[p & 1][(p >> 1) % len((xs, os_)[p & 1])] for p in range(2 * n)]
        boards = []
        for r in line:
            x, o, _ = r.board.masks()
            boards.append([1 if x & int(b) else 2 if o & int(b) else 0 for b in link._CELL_BIT])
        entries.append({"boards": boards, "moves": [["c", [0, 0]]] * len(line), "result": 1 + len(entries) % 2,
                        "blockers": link.blockers_to_cells(mask)})
        roots.append(line)
    return entries, roots


def check_deep_rows_walls_budgets():
    entries, roots = deep_entries()
    a = link.entries_to_arrays(entries)
    assert len(set(a.blockers.tolist())) == len(entries) >= 7 and 0 not in a.blockers.tolist()
    flat = [r for line in roots for r in line]
    short = {}
    for depth, budget in ((6, 256), (6, 1 << 12), (8, 256), (8, 1 << 16)):
        store = link.SampleStore(len(a.games), len(a.ply_flags), len(a.target_index))
        store.add_arrays(a)
        pairs = eligible_pairs(store)
        assert len(pairs) == len(flat) >= 210
        packed, walls = positions(store, pairs)
        for k, r in enumerate(flat):                                       # the stored ply is the fixture's root
            assert (int(packed[k][0]), int(packed[k][1])) == tuple(r.board.packed()) and int(walls[k]) == r.board.masks()[2], k
        out = link.alphabeta_search(packed, walls, depth, budget)
        stats = store.prove(0, len(entries), depth, budget)                # every wall mask in one call
        same_as_search(store, pairs, out, (depth, budget))
        assert stats == recount(store, pairs, out, False), (depth, budget, stats)
        proof, move, done = store.proofs(pairs)
        for k, r in enumerate(flat):
            if rr.result(r.board) != 0:
                assert (int(move[k]), int(done[k])) == (NO_MOVE, depth) and abs(int(proof[k])) == WIN + depth, k
            else:
                assert 1 <= done[k] <= depth, k
                want_move, want_value, _ = r.answers[int(done[k]) - 1]
                assert (int(move[k]), int(out.values[k])) == (want_move, want_value), (depth, budget, k, r.board.fen())
        short[depth, budget] = int((done < depth).sum())
        assert stats["wins"] > 0 and stats["losses"] > 0 and stats["contradicted"] > 0
        store.close()
    assert short[6, 256] > 0 and short[8, 256] > 0, short                  # a budget of 256 abandons iterations
    assert short[8, 1 << 16] < short[8, 256], short


def batches(store, draws, seed):
    """Every minibatch the checks compare: gather and draw_gather, value_blend 0 and 0.5, without and with the auxiliary outputs
    -> {name: arrays}; a draw_gather's draws ride along as its last array"""
    out = {}
    for blend in (0.0, 0.5):
        for aux in (False, True):
            out["gather", blend, aux] = host(store.gather(draws, blend, aux=aux))
            drawn = torch.zeros((len(draws), 4), dtype=torch.int32, device="cuda")
            got = store.draw_gather(len(draws), seed, 3, 0, store.counts()["games"], blend, draws_out=drawn, aux=aux)
            out["draw_gather", blend, aux] = host(got) + (drawn.cpu().numpy(),)
    assert store.status() == 0
    return out


def compare_batches(store, before, after, draws, retargeted=()):
    """Bit-identical, except the value of a sample on a proven ply (+-1 by the proof's sign) and, for the plies of `retargeted`
    = {(game, ply): move}, the policy row (the one-hot of the move under the sample's symmetry) and the reply row of the ply
    before it, which is that ply's policy target -> the proven samples met"""
    met = {"proven": 0, "contradicted": 0, "retargeted": 0, "replies": 0, "blended": 0}
    games, _ = store.mirror()
    for key in before:
        b, a = before[key], after[key]
        rows = np.asarray(draws)[:, :3] if key[0] == "gather" else a[-1][:, :3]
        if key[0] == "draw_gather":
            assert a[-1].tobytes() == b[-1].tobytes(), key                  # the draws do not move
        proof = store.proofs(rows[:, :2])[0]
        for t in range(len(b) - (key[0] == "draw_gather")):
            if t == 2:                                                       # value (n, 1)
                for k, (g, p, s) in enumerate(rows.tolist()):
                    if proof[k]:
                        assert a[2][k].tobytes() == np.float32(1.0 if proof[k] > 0 else -1.0).tobytes(), (key, g, p)
                        met["proven"] += 1
                        met["contradicted"] += (proof[k] > 0) != ((int(games[g][2]) & 0xFF) == 1 + (p & 1))
                        met["blended"] += abs(float(b[2][k, 0])) != 1.0
                    else:
                        assert a[2][k].tobytes() == b[2][k].tobytes(), (key, g, p)
            elif t in (1, 5) and retargeted:                                 # policy, and the reply: ply p + 1's policy target
                for k, (g, p, s) in enumerate(rows.tolist()):
                    q = (g, p + (t == 5))
                    if q in retargeted:
                        want = np.zeros(833, dtype=np.float32)
                        want[link.symmetry_policy_index(s, policy_index(retargeted[q]))] = 1.0
                        assert a[t][k].tobytes() == want.tobytes(), (key, t, g, p, s)
                        met["retargeted" if t == 1 else "replies"] += 1
                    else:
                        assert a[t][k].tobytes() == b[t][k].tobytes(), (key, t, g, p)
            else:
                assert a[t].tobytes() == b[t].tobytes(), (key, t)
    return met


def chosen_draws(store):
    """The last 20 plies of every game and every seventh ply before them, the symmetries in turn"""
    games, _ = store.mirror()
    picks = [(g, p) for g in range(len(games)) for p in range(int(games[g][1]))
             if p >= int(games[g][1]) - 20 or p % 7 == 0]
    return np.array([(g, p, k % 8) for k, (g, p) in enumerate(picks)], dtype=np.int32)


def check_minibatches():
    store = golden_store()
    draws = chosen_draws(store)
    before = batches(store, draws, seed=99)
    assert compare_batches(store, before, batches(store, draws, seed=99), draws)["proven"] == 0
    stats = store.prove(0, 6, 3)
    assert stats["wins"] + stats["losses"] > 0 and stats["retargeted"] == 0
    met = compare_batches(store, before, batches(store, draws, seed=99), draws)
    assert met["proven"] >= 4 * 26 and met["contradicted"] >= 4 * 14 and met["blended"] > 0, met
    drawn = before["draw_gather", 0.0, False][-1][:, :2]
    assert (store.proofs(drawn)[0] != 0).any()                               # the device's own draws met a proven ply too
    store.close()
    # with retarget_wins: the policy row of a proven win, the placement, and a game added behind the new pairs
    store = golden_store(spare_targets=1351, room=1)
    before = batches(store, draws, seed=99)
    pairs = eligible_pairs(store)
    t0 = store.counts()["targets"]
    stats = store.prove(0, 6, 3, retarget_wins=True)
    proof, move, done = store.proofs(pairs)
    won = [(pairs[k], int(move[k])) for k in range(len(pairs)) if proof[k] > 0 and move[k] != NO_MOVE]
    assert stats["retargeted"] == len(won) > 20 and store.counts()["targets"] == t0 + len(won)
    where = store.ply_targets([p for p, _ in won])
    assert where.tolist() == [[t0 + rank, 1] for rank in range(len(won))]     # in visiting order
    lost = [pairs[k] for k in range(len(pairs)) if proof[k] < 0]
    _, _, _, start, index, weight = store.read_plies([p for p, _ in won])
    assert index.tolist() == [policy_index(mv) for _, mv in won] and weight.tolist() == [1.0] * len(won)
    met = compare_batches(store, before, batches(store, draws, seed=99), draws, {tuple(p): mv for p, mv in won})
    assert met["retargeted"] >= 4 * 22 and met["replies"] >= 22 and met["proven"] > met["retargeted"] and len(lost) > 0, met
    store.add_entries(golden_entries()[1:2])                               # 235 plies, one target each
    assert store.ply_targets([(6, 0)])[0][0] == t0 + len(won)
    assert store.proofs([(6, 0), (6, 100)])[0].tolist() == [0, 0]
    store.close()


def check_monotone():
    store = golden_store()
    pairs = eligible_pairs(store)
    first = store.prove(0, 6, 2)
    proven = first["wins"] + first["losses"]
    assert first["visited"] == len(pairs) and proven > 0
    words = store.proofs(pairs)
    assert int((words[0] != 0).sum()) == proven
    again = store.prove(0, 6, 1)                                             # a smaller depth: nothing new
    assert again["visited"] == len(pairs) - proven and again["wins"] == again["losses"] == again["contradicted"] == 0
    assert store.proofs(pairs)[0].tolist() == words[0].tolist()
    was = words[0] != 0
    for k in (1, 2):                                                         # a proven ply keeps its move and iteration too
        assert store.proofs(pairs)[k][was].tolist() == words[k][was].tolist()
    deeper = store.prove(0, 6, 3)
    assert deeper["visited"] == len(pairs) - proven and deeper["wins"] + deeper["losses"] > 0
    now = store.proofs(pairs)
    assert now[0][was].tolist() == words[0][was].tolist() and int((now[0] != 0).sum()) == proven + deeper["wins"] + deeper["losses"]
    for k in (1, 2):
        assert now[k][was].tolist() == words[k][was].tolist()
    # a part of the games: only theirs are visited
    part = golden_store()
    games, _ = part.mirror()
    some = part.prove(2, 3, 1)
    assert some["visited"] == int(games[2:5, 1].sum())
    proof = part.proofs(all_pairs(part))[0]
    outside = np.array([g < 2 or g >= 5 for g, _ in all_pairs(part).tolist()])
    assert not proof[outside].any() and proof[~outside].any()
    part.close()
    store.close()


def check_refusals():
    store = golden_store()                                                   # no spare targets
    pairs, draws = all_pairs(store), chosen_draws(store)
    before, counts = batches(store, draws, seed=5), store.counts()

    def refused(code, *args, **kw):
        try:
            store.prove(*args, **kw)
        except link.AzhError as err:
            assert "error %d" % code in str(err), err
        else:
            raise AssertionError("the call was accepted: %r %r" % (args, kw))
        proof, move, done = store.proofs(pairs)
        assert not proof.any() and set(move.tolist()) == {NO_MOVE} and not done.any()
        assert store.counts() == counts
        after = batches(store, draws, seed=5)
        for key in before:
            for b, a in zip(before[key], after[key]):
                assert a.tobytes() == b.tobytes(), (key, args)

    refused(-2, 0, 6, 0)
    refused(-2, 0, 6, 9)
    refused(-2, 0, 6, 4)                                                     # no budget past depth 3
    refused(-2, 0, 6, 3, 100)                                                # a budget below MAX_MOVES
    refused(-1, 0, 7, 3)
    refused(-1, 5, 2, 3)
    refused(-1, -1, 2, 3)
    refused(-1, 0, 0, 3)
    refused(-1, 0, 7, 9)                                                     # the range is looked at first
    refused(-6, 0, 6, 3, retarget_wins=True)                                 # the searches ran; nothing was committed
    assert store.prove(0, 6, 3)["wins"] > 0                                  # and the same call without the pairs goes through
    store.close()


CHECKS = [check_proofs_are_the_searchs, check_deep_rows_walls_budgets, check_minibatches, check_monotone, check_refusals]


if __name__ == "__main__":
    fresh_process.main(CHECKS)
