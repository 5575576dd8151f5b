"""Policy surprise weighting, the parts that need no device: one ply's surprise (azh_samples_surprise_host) against a float64
restatement, the weighted draw (azh_samples_draw with candidates and cum) against a restatement in Python integers on the oracle's Philox, and
training.surprise_weights."""
import numpy as np
import pytest

from ataxxzero_amd import link, training
from tests import surprise_reference as ref
from tests.surprise_reference import BAD, PASS, edge_specs

F32 = np.float32
SEED = 0x1234567_89ABCDEF


@pytest.fixture(scope="module")
def views():
    return ref.fixture_views()


def test_the_host_movegen_gives_the_oracles_moves_in_its_order(views):
    counts = set()
    for mover, opponent, _, legal in views:
        assert list(link.samples_legal(mover, opponent)) == legal
        counts.add(len(legal))
    assert {0, 1, 64, 65} <= counts and max(counts) > 128


def test_surprise_against_float64(views):
    """|f32 - float64| <= the bound surprise_reference.kl_reference derives from the det-math ulp bounds (0.85 ulp logf, 1.05 ulp
    expf: tests/test_detmath_accuracy.py) and the term counts; for the cases here, logits ~ 3 N(0, 1) and up to 40 targets, it
    comes to between 1e-7 and 2e-5 — printed below with the worst error met."""
    rng = np.random.default_rng(11)
    worst, bounds, n = 0.0, [], 0
    for mover, opponent, _, legal in views[::7]:
        if not legal:
            continue
        logits = (3.0 * rng.standard_normal(833)).astype(F32)
        k = int(rng.integers(1, min(len(legal), 40) + 1))
        t_index = rng.choice(legal, size=k, replace=False)
        t_weight = rng.dirichlet(np.ones(k)).astype(F32)
        t_weight[t_weight <= 0] = F32(1e-6)
        got, illegal = link.samples_surprise_host(logits, legal, t_index, t_weight)
        want, want_illegal, bound = ref.kl_reference(logits, legal, t_index, t_weight)
        assert illegal == want_illegal == 0
        assert np.isfinite(got) and got >= 0
        assert abs(float(got) - want) <= bound, (float(got), want, bound, len(legal), k)
        worst, n = max(worst, abs(float(got) - want)), n + 1
        bounds.append(bound)
    print("surprise: %d plies, worst |f32 - f64| %.3e, bounds %.3e .. %.3e" % (n, worst, min(bounds), max(bounds)))
    assert n > 200 and max(bounds) < 1e-4


def test_surprise_edge_cases(views):
    by_count = {}
    for v in views:
        by_count.setdefault(len(v[3]), v)
    rng = np.random.default_rng(5)
    logits = rng.standard_normal(833).astype(F32)
    # one legal move, a one-hot target on it: log p is exactly 0 and so is the KL
    legal = by_count[1][3]
    assert link.samples_surprise_host(logits, legal, legal, [1.0]) == (F32(0.0), 0)
    legal = by_count[65][3]
    # a target of weight 0 adds nothing, legal or not, and is not counted
    base = link.samples_surprise_host(logits, legal, legal[:3], [0.5, 0.25, 0.25])
    other = next(i for i in range(833) if i not in legal)
    assert link.samples_surprise_host(logits, legal, legal[:3] + [legal[9], other], [0.5, 0.25, 0.25, 0.0, 0.0]) == base
    assert base[0] > 0 and base[1] == 0
    # all-equal logits: the prior is uniform, KL = ln n - H(target)
    got, _ = link.samples_surprise_host(np.full(833, 0.25, F32), legal, legal[:2], [0.5, 0.5])
    want, _, bound = ref.kl_reference(np.full(833, 0.25, F32), legal, legal[:2], [0.5, 0.5])
    assert abs(float(got) - want) <= bound and abs(want - (np.log(65) - np.log(2))) < 1e-12
    # a target that is no legal move adds nothing and is counted
    got = link.samples_surprise_host(logits, legal, [legal[0], other, legal[1]], [0.5, 0.25, 0.25])
    want, want_illegal, bound = ref.kl_reference(logits, legal, [legal[0], other, legal[1]], [0.5, 0.25, 0.25])
    assert got[1] == want_illegal == 1 and abs(float(got[0]) - want) <= bound
    # hostile logits: the stored value is 0 or finite, never a NaN
    for value in (3e38, -3e38, np.inf, -np.inf, np.nan):
        for where in ("all", "target", "other", "legal"):
            hostile = logits.copy()
            if where == "all":
                hostile[:] = value
            elif where == "target":
                hostile[legal[0]] = value
            elif where == "other":
                hostile[legal[5]] = value
            else:
                hostile[legal] = value
            got, illegal = link.samples_surprise_host(hostile, legal, legal[:3], [0.5, 0.25, 0.25])
            assert np.isfinite(got) and got >= 0 and illegal == 0, (value, where, got)
    assert link.samples_surprise_host(np.full(833, np.nan, F32), legal, legal[:3], [0.5, 0.25, 0.25])[0] == 0
    # no legal move at all (a pass position that carries a target): nothing is legal
    assert link.samples_surprise_host(logits, [], legal[:2], [0.5, 0.5]) == (F32(0.0), 2)


# ---------------------------------------------------------------- the weighted draw


def test_weighted_draw_equals_the_integer_restatement():
    rng = np.random.default_rng(21)
    games, flags, cand, cum = ref.build_mirror(edge_specs(rng))
    g_list, f_list, lists, cums = ref.per_game_lists(games, flags, cum)
    assert cums[2][-1] == 0 and lists[1] == [] and len(lists[5]) == 4096 and cums[9][-1] > 1 << 31
    zero_weight = {(g, p) for g in range(len(g_list)) for k, p in enumerate(lists[g])
                   if cums[g][k] == (cums[g][k - 1] if k else 0)}
    assert (3, 8) in zero_weight and (3, 0) in zero_weight
    seen, pairs = set(), 0
    for step in range(40):
        for i in range(250):                                              # 10^4 (step, sample) pairs
            first, count = (0, len(g_list)) if step % 2 == 0 else (3, 6)      # every game; a window with first_game > 0
            got = link.samples_draw_weighted(SEED, step, i, first, count, games, flags, cand, cum)
            assert got == ref.restated_weighted_draw(SEED, step, i, first, count, g_list, f_list, lists, cums), (step, i)
            g, ply, sym, attempts = got
            assert g >= first and g < first + count and 0 <= sym < 8 and 1 <= attempts <= 64
            assert g not in (1, 2)                                        # no candidate; total 0
            assert not f_list[g_list[g][0] + ply] & (PASS | BAD)
            if g_list[g][3]:
                assert ply == g_list[g][3]
            else:
                assert (g, ply) not in zero_weight and ply in lists[g]
            seen.add((g, ply))
            pairs += 1
    assert pairs == 10 ** 4
    assert {g for g, _ in seen} == {0, 3, 4, 5, 6, 7, 8, 9}
    assert {p for g, p in seen if g == 3} == {1, 4, 5} and {p for g, p in seen if g == 6} == {1, 5}
    assert len({p for g, p in seen if g == 5}) > 300
    # ranges that cannot give a sample exhaust the attempts
    assert link.samples_draw_weighted(SEED, 0, 0, 1, 2, games, flags, cand, cum) == (-1, -1, -1, 64)
    with pytest.raises(link.AzhError):
        link.samples_draw_weighted(SEED, 0, 0, 5, 6, games, flags, cand, cum)


def test_the_draw_takes_candidates_and_cum_together_or_not_at_all():
    """azh_samples_draw called as the library exports it: with one of the two mirrors it returns -1; with both its rows are the
    weighted restatement's, with neither the uniform one's."""
    from tests.samples_fixtures import restated_draw
    games, flags, cand, cum = ref.build_mirror(edge_specs(np.random.default_rng(21)))
    g_list, f_list, lists, cums = ref.per_game_lists(games, flags, cum)
    out = np.full(4, 77, dtype=np.int32)

    def draw(step, i, first, count, candidates, sums):
        return link.load().azh_samples_draw(SEED, step, i, first, count, games.ctypes.data, len(games), flags.ctypes.data,
                                            link._ptr(candidates), link._ptr(sums), out.ctypes.data)
    assert draw(0, 0, 0, len(g_list), cand, None) == -1 and draw(0, 0, 0, len(g_list), None, cum) == -1
    assert out.tolist() == [77] * 4
    for step in range(2):
        for i in range(100):
            first, count = (0, len(g_list)) if step == 0 else (3, 6)
            assert draw(step, i, first, count, cand, cum) == 0
            assert tuple(out.tolist()) == ref.restated_weighted_draw(SEED, step, i, first, count, g_list, f_list, lists, cums)
            assert draw(step, i, first, count, None, None) == 0
            assert tuple(out.tolist()) == restated_draw(SEED, step, i, first, count, games, flags)


@pytest.mark.parametrize("units", [65536, 7, 1])
def test_equal_weights_are_the_uniform_draw(units):
    """floor(floor(v c q / 2^32) / q) = floor(v c / 2^32) for every q >= 1: the rows are azh_samples_draw's."""
    from tests.samples_fixtures import draw_mirror
    games, flags, _ = draw_mirror()
    specs = [([int(f) for f in flags[first:first + plies]], int(word), int(r1), None)
             for first, plies, word, r1 in games.tolist()]
    games2, flags2, cand, cum = ref.build_mirror(specs)
    assert (games2 == games).all() and (flags2 == flags).all()
    cum = (cum.astype(np.uint64) // 65536 * units).astype(np.uint32)
    for step in range(4):
        for i in range(257):
            assert link.samples_draw_weighted(SEED, step, i, 0, 40, games, flags, cand, cum) == \
                link.samples_draw(SEED, step, i, 0, 40, games, flags)
    for i in range(64):
        assert link.samples_draw_weighted(SEED, 9, i, 10, 30, games, flags, cand, cum) == \
            link.samples_draw(SEED, 9, i, 10, 30, games, flags)


# ---------------------------------------------------------------- training.surprise_weights

def test_surprise_weights():
    rng = np.random.default_rng(3)
    games, lists, at = [], [], 0
    for g in range(30):
        plies = int(rng.integers(1, 50))
        cand = sorted(rng.choice(plies, size=int(rng.integers(0, plies + 1)), replace=False).tolist())
        games.append((at, plies, 1, 0))
        lists.append(cand)
        at += plies
    kl = rng.random(at)
    for g in (3, 4):                                                      # games whose candidates all have KL 0
        kl[games[g][0]:games[g][0] + games[g][1]] = 0
    for lam in (0.0, 0.5, 1.0):
        w = training.surprise_weights(kl, games, lists, lam)
        assert w.dtype == np.float64 and w.shape == (at,) and (w >= 0).all()
        for (first, plies, _, _), cand in zip(games, lists):
            mine = w[first:first + plies]
            assert mine.sum() == pytest.approx(len(cand), rel=1e-12)      # the game's mass is its candidate count
            assert (np.delete(mine, cand) == 0).all()                     # non-candidates get 0
            if lam == 0.0 or kl[first:first + plies][cand].sum() == 0:
                assert (mine[cand] == 1).all()
            elif cand:
                k = kl[first:first + plies][cand]
                assert np.allclose(mine[cand], (1 - lam) + lam * len(cand) * k / k.sum(), rtol=1e-12)
    assert (training.surprise_weights(kl, games, lists, 1.0)[lists[0]] >= 0).all()
    with pytest.raises(ValueError):
        training.surprise_weights(kl, games, lists, 1.5)
