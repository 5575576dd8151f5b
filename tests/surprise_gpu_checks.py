"""The device checks of tests/test_gpu_surprise.py, run in a process of their own for the reason tests/samples_gpu_checks.py
gives: torch's runtime must be loaded first.  `python -m tests.surprise_gpu_checks OUT.json` runs every check and writes
{name: "ok" | traceback}; after a check that ends in a device error nothing more is run."""
import numpy as np
import torch

from ataxxzero_amd import link, model
from oracle import net_oracle
from tests import fresh_process
from tests import surprise_reference as ref
from tests.store_checks import arrays_of, host, same, store_of
from tests.surprise_reference import BAD, FULL, PASS
from tests.surprise_reference import edge_specs

F32 = np.float32
HOSTILE = (3e38, -3e38, np.inf, -np.inf, np.nan)


def unwalled(games):
    """games: [[ply] per game] as tests/store_checks.py::arrays_of takes them: every game without a wall mask"""
    return [(None, plies) for plies in games]


def seam_plies():
    """About 40 plies on the kernel's seams: 1, 64, 65 and 129 legal moves; 1, 63, 64, 65 and 130 targets (the 130th is no
    legal move: the position with the most moves among the fixtures has 129); a pass; a bad ply."""
    rng = np.random.default_rng(17)
    by_count, rich = {}, []
    for v in ref.fixture_views():
        by_count.setdefault(len(v[3]), v)
        if len(v[3]) >= 66:
            rich.append(v)
    assert {1, 64, 65, 129} <= set(by_count)
    assert [len(link.samples_legal(by_count[n][0], by_count[n][1])) for n in (1, 64, 65, 129)] == [1, 64, 65, 129]

    def ply(view, k, extra=0, flags=0, scale=1.0):
        mover, opponent, _, legal = view
        chosen = [int(i) for i in rng.choice(legal, size=k, replace=False)]
        chosen += [i for i in range(833) if i not in legal][:extra]
        w = (rng.dirichlet(np.ones(len(chosen))) * scale).astype(F32)
        return mover, opponent, flags, chosen, w

    plies = [ply(by_count[1], 1), ply(by_count[64], 1), ply(by_count[64], 63), ply(by_count[64], 64), ply(by_count[65], 64),
             ply(by_count[65], 65), ply(by_count[129], 65), ply(by_count[129], 129, extra=1), ply(by_count[129], 128),
             (by_count[65][0], by_count[65][1], PASS, [], []), ply(by_count[65], 5, scale=0.5),
             ply(by_count[65], 3, extra=2)]
    while len(plies) < 40:
        v = rich[int(rng.integers(len(rich)))]
        plies.append(ply(v, int(rng.integers(1, 66))))
    return plies


# ---------------------------------------------------------------- the checks

def check_from_logits_bit_exact():
    plies = seam_plies()
    games = [plies[:7], plies[7:8], plies[8:]]               # three games: the mover follows the ply's parity in its game
    a = arrays_of(unwalled(games))
    store = store_of(a)
    flags = store.mirror()[1]
    assert store.counts()["bad_plies"] == 1 and int(flags[9]) & PASS and int(flags[10]) & BAD
    rng = np.random.default_rng(23)
    n = len(plies)
    logits = (3.0 * rng.standard_normal((n, 833))).astype(F32)
    for i in range(12, 12 + 3 * len(HOSTILE)):               # hostile values: every logit, the first target's, a legal move's
        value, where = HOSTILE[(i - 12) % len(HOSTILE)], (i - 12) // len(HOSTILE)
        legal = link.samples_legal(plies[i][0], plies[i][1])
        if where == 0:
            logits[i, :] = value
        elif where == 1:
            logits[i, plies[i][3][0]] = value
        else:
            logits[i, [j for j in legal if j not in plies[i][3]][:1] or legal[:1]] = value
    want, want_illegal = np.zeros(n, dtype=F32), np.zeros(n, dtype=np.int64)
    for i, (mover, opponent, f, t_index, t_weight) in enumerate(plies):
        if int(flags[i]) & (PASS | BAD):
            continue
        want[i], want_illegal[i] = link.samples_surprise_host(logits[i], link.samples_legal(mover, opponent), t_index, t_weight)
    assert want_illegal[7] == 1 and want_illegal[11] == 2 and want_illegal.sum() == 3
    assert not np.isnan(want).any() and (want[:9] > 0).sum() >= 8 and want[0] == 0 and (want[12:] > 0).sum() > 10
    dev = torch.from_numpy(logits).cuda()
    for first, last in ((0, n), (3, n), (8, 9), (0, 8), (n - 1, n)):
        got, illegal = store.surprise_from_logits(first, dev[first:last].contiguous())
        assert got.dtype == F32 and got.tobytes() == want[first:last].tobytes(), (first, last, got, want[first:last])
        assert illegal == want_illegal[first:last].sum(), (first, last)
    for bad_range in ((n, 1), (n - 1, 2), (-1, 1)):
        try:
            store.surprise_from_logits(bad_range[0], dev[:bad_range[1]].contiguous())
        except link.AzhError:
            pass
        else:
            raise AssertionError("plies %r were accepted" % (bad_range,))
    store.close()


def check_net_surprise():
    """surprise(net, f32) against the float64 tower and the float64 restatement.  KL is 2-Lipschitz in the logits under the sup
    norm (the weights sum to 1 and each log p_t moves by at most twice the logits' error), so the bound is 2 x the f32 tower's
    pinned 1e-5 plus the arithmetic bound kl_reference derives.  The net is 2 blocks x 64 filters: the narrowest tower built."""
    rng = np.random.default_rng(31)
    views = [v for v in ref.fixture_views() if len(v[3]) >= 2]
    picked = [views[int(i)] for i in rng.choice(len(views), size=64, replace=False)]
    plies = []
    for mover, opponent, _, legal in picked:
        k = int(rng.integers(1, min(len(legal), 30) + 1))
        plies.append((mover, opponent, 0, rng.choice(legal, size=k, replace=False), rng.dirichlet(np.ones(k)).astype(F32)))
    games = [plies[:5], plies[5:37], plies[37:38], plies[38:]]
    store = store_of(arrays_of(unwalled(games)))
    conv, bn = model.random_init(2, 64, seed=7, perturb_bn=True)
    net = link.Net(conv, bn)
    got, illegal = store.surprise(net, link.DTYPE_F32, 0, 4)
    assert illegal == 0 and got.shape == (64,) and got.dtype == F32
    small, _ = store.surprise(net, link.DTYPE_F32, 0, 4, chunk=16)           # four launches: the chunk seam is crossed
    assert small.tobytes() == got.tobytes()
    odd, _ = store.surprise(net, link.DTYPE_F32, 0, 4, chunk=27)             # the last chunk is a short one
    assert odd.tobytes() == got.tobytes()
    part, _ = store.surprise(net, link.DTYPE_F32, 1, 2, chunk=16)            # a window of games
    assert part.tobytes() == got[5:38].tobytes()
    ms = store.surprise_ms()
    assert ms[0] > 0 and ms[1] > 0
    boards = np.array([(p[0], p[1]) for p in plies], dtype=np.uint64)
    ref_logits, _ = net_oracle.forward(conv, bn, net_oracle.features_from_leaf_boards(boards, 0))
    ref_logits = ref_logits.reshape(64, 833)
    worst = 0.0
    for i, (mover, opponent, _, t_index, t_weight) in enumerate(plies):
        want, _, bound = ref.kl_reference(ref_logits[i], link.samples_legal(mover, opponent), t_index, t_weight)
        err = abs(float(got[i]) - want)
        worst = max(worst, err)
        assert err <= 2 * 1e-5 + bound, (i, float(got[i]), want, bound)
    print("surprise(net, f32) on 64 positions: worst |device - float64| %.3e, KL %.4f .. %.4f" % (worst, got.min(), got.max()))
    # the 16-bit towers give the same plies about the same surprise
    low, _ = store.surprise(net, link.DTYPE_BF16, 0, 4)
    assert np.abs(low - got).max() < 0.25 * max(1.0, float(got.max()))
    net.close()
    store.close()
    return worst


def weighted_store():
    """A store holding the games of tests/test_surprise_host.py::edge_specs with random boards and one-hot targets, and the
    mirrors build_mirror makes of them."""
    rng = np.random.default_rng(21)
    specs = edge_specs(rng)
    games = []
    for ply_flags, word, r1, _ in specs:
        plies = []
        for f in ply_flags:
            x = int(rng.integers(0, 1 << 49))
            o = int(rng.integers(0, 1 << 49)) & ~x
            weight = [] if f & PASS else [0.5 if f & BAD else 1.0]
            plies.append((x, o, f & (PASS | FULL), [int(rng.integers(833))] * len(weight), weight))
        games.append(plies)
    a = arrays_of(unwalled(games))
    a.games[:, 2] = [s[1] for s in specs]
    a.games[:, 3] = [s[2] for s in specs]
    return specs, a


def per_ply_weights(specs, lo, hi):
    return np.concatenate([np.ones(len(s[0]), F32) if s[3] is None else np.asarray(s[3], F32) for s in specs[lo:hi]])


def check_weighted_draws():
    specs, a = weighted_store()
    store = store_of(a, spare=64)
    games, flags, cand, cum = ref.build_mirror(specs)
    assert (store.mirror()[0] == games).all()
    assert (store.mirror()[1] == np.where(flags & PASS, flags | BAD, flags)).all()      # (a pass has no target: bad as well)
    count = np.array([len(ref.candidates_of(int(g[0]), int(g[1]), int(g[2]), flags)) for g in games])
    n, G = 256, len(specs)
    draws_out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")

    def valid(c):                                            # a cum array below each game's candidate count
        return np.concatenate([c[int(g[0]):int(g[0]) + k] for g, k in zip(games, count)])

    def drawn(step, first=0, n_games=G):
        out = host(store.draw_gather(n, 77, step, first, n_games, 0.0, draws_out=draws_out))
        return out, draws_out.cpu().numpy().copy()

    uniform = [drawn(step)[1] for step in range(3)]          # the unweighted kernel, before any weight is held
    got_cand, got_count, got_cum, present = store.ply_cum()
    assert not present and (got_count == count).all() and (valid(got_cand) == valid(cand)).all()
    assert (valid(got_cum) == np.concatenate([65536 * np.arange(1, k + 1) for k in count])).all()
    # all-ones weights: the same draws, row for row
    store.set_ply_weights(0, G, np.ones(len(flags), F32))
    assert store.ply_cum()[3] and (valid(store.ply_cum()[2]) == valid(got_cum)).all()
    for step in range(3):
        assert (drawn(step)[1] == uniform[step]).all(), step
    # the games' own weights; game 7 is never given any.  The rounding rule: q = floor(w * 65536 + 0.5), as build_mirror has it
    store.set_ply_weights(0, 7, per_ply_weights(specs, 0, 7))
    store.set_ply_weights(8, 2, per_ply_weights(specs, 8, 10))
    held = store.ply_cum()[2].copy()
    assert (valid(held) == valid(cum)).all()
    assert ref.weight_units(1e-6) == 0 and ref.weight_units(0.25) == 16384 and ref.weight_units(F32(2.0 ** -17)) == 1
    # refusals change nothing
    w = per_ply_weights(specs, 0, G)
    for at, value in ((5, np.nan), (5, -1.0), (5, np.inf), (0, -0.5)):
        refused = w.copy()
        refused[at] = value
        try:
            store.set_ply_weights(0, G, refused)
        except link.AzhError as err:
            assert "error -1" in str(err), err
        else:
            raise AssertionError("a weight of %r was accepted" % (value,))
        assert (store.ply_cum()[2] == held).all()
    first9 = int(games[9][0])
    for heavy in ([65535.0, 65535.0, 1.0], [40000.0, 30000.0, 0.0]):     # game 9: more than 2^32 - 1 units in all
        refused = w.copy()
        refused[first9:first9 + 3] = heavy
        try:
            store.set_ply_weights(0, G, refused)
        except link.AzhError as err:
            assert "error -1" in str(err), err
        else:
            raise AssertionError("an overflowing game was accepted")
        assert (store.ply_cum()[2] == held).all()
    # the weighted draws: the host restatement's rows, gather()'s minibatch, never a ply without weight
    g_list, f_list, lists, cums = ref.per_game_lists(games, flags, cum)
    zero = {(g, p) for g in range(G) for k, p in enumerate(lists[g]) if cums[g][k] == (cums[g][k - 1] if k else 0)}
    seen = set()
    for step, (first, n_games) in enumerate([(0, G), (3, 6), (0, G)]):
        out, draws = drawn(step, first, n_games)
        for i in range(n):
            row = tuple(int(v) for v in draws[i])
            assert row == store.draw_weighted(77, step, i, first, n_games), (step, i)
            assert row == ref.restated_weighted_draw(77, step, i, first, n_games, g_list, f_list, lists, cums), (step, i)
            g, ply = row[:2]
            assert first <= g < first + n_games and g not in (1, 2)
            assert ply == g_list[g][3] if g_list[g][3] else (g, ply) not in zero
            seen.add((g, ply))
        same(out, host(store.gather(draws[:, :3], 0.0)))
    assert {g for g, _ in seen} == {0, 3, 4, 5, 6, 7, 8, 9} and {1, 5} <= {p for g, p in seen if g == 3} <= {1, 4, 5}
    assert any((d != u).any() for d, u in ((drawn(0)[1], uniform[0]), (drawn(2)[1], uniform[2])))
    assert store.status() == 0
    # a game added while weights are held weighs one per candidate
    extra = arrays_of(unwalled([[(1, 2, 0, [5], [1.0])] * 4]))
    store.add_arrays(extra)
    c2, k2, cum2, _ = store.ply_cum()
    assert k2[-1] == 4 and list(cum2[-4:]) == [65536, 131072, 196608, 262144] and (cum2[:-4] == held).all()
    _, draws = drawn(5, G, 1)
    assert (draws[:, 0] == G).all() and set(draws[:, 1].tolist()) == {0, 1, 2, 3}
    # cleared: the unweighted kernel path again
    store.clear_ply_weights()
    assert not store.ply_cum()[3]
    for step in range(3):
        assert (drawn(step)[1] == uniform[step]).all(), step
    assert store.status() == 0
    store.close()


CHECKS = [check_from_logits_bit_exact, check_net_surprise, check_weighted_draws]


if __name__ == "__main__":
    fresh_process.main(CHECKS)
