"""The host arithmetic of the Gumbel root search (azh_gumbel_considered_visits, azh_gumbel_noise, azh_gumbel_root; no device)
against the numpy restatement tests/gumbel_reference.py, bit for bit, and the properties of the restatement itself: a
simulated search always finds a candidate and visits at most min(m, M) root edges, the played edge has the most visits, the
arg-max of the improved policy is written as 65535, a better score never lowers an edge's count, and c_scale -> 0+ gives the
prior back."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import link
from tests import gumbel_reference as gr

F32 = np.float32
SEED = 0x1234ABCD5678
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("r", [1, 2, 3, 4, 16, 17, 64, 256])
@pytest.mark.parametrize("V", [1, 2, 7, 16, 33, 100])
def test_considered_visits_equal_the_schedule(r, V):
    want = gr.seq(r, V)
    assert len(want) == V
    assert link.gumbel_considered_visits(r, V).tolist() == want


def test_the_schedule_of_the_paper_at_16_actions_and_32_simulations():
    """16 actions once (a phase is never shorter than one round), 8 once more, 4 twice: the budget ends in the third phase;
    at 64 simulations every phase has its 16 and the last two actions get four rounds"""
    assert gr.seq(16, 32) == [0] * 16 + [1] * 8 + [2] * 4 + [3] * 4
    assert gr.seq(16, 64) == [0] * 16 + [1] * 8 + [2] * 8 + [3] * 4 + [4] * 4 + [5] * 4 + [6] * 4 + [7] * 2 + [8] * 2 + \
        [9] * 2 + [10] * 2 + [11] * 2 + [12] * 2 + [13] * 2 + [14] * 2
    assert gr.seq(1, 5) == [0, 1, 2, 3, 4] and gr.seq(2, 5) == [0, 0, 1, 1, 2]


@pytest.mark.parametrize("bad", [(0, 8), (257, 8), (4, 0), (4, 60001)])
def test_considered_visits_refuse_what_is_out_of_range(bad):
    with pytest.raises(link.AzhError):
        link.gumbel_considered_visits(*bad)


def test_noise_equals_the_probes_bit_for_bit():
    for uid, ply, M in [(0, 0, 1), (7, 3, 64), (123456, 399, 256), (0xFFFFFFFF, 0, 65)]:
        got = link.gumbel_noise(SEED, uid, ply, M)
        want = gr.noise(SEED, uid, ply, M)
        assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all()
        assert np.isfinite(got).all()
    # a Gumbel(0, 1) sample: mean 0.5772, variance pi^2 / 6 (4096 draws: standard error of the mean 0.02)
    g = np.concatenate([link.gumbel_noise(SEED, u, 0, 256) for u in range(16)]).astype(np.float64)
    assert abs(g.mean() - 0.5772) < 0.1 and abs(g.var() - np.pi ** 2 / 6) < 0.25
    assert len(link.gumbel_noise(SEED, 1, 1, 0)) == 0
    with pytest.raises(link.AzhError):
        link.gumbel_noise(SEED, 1, 1, 257)


def _synthetic_root(rng, M, N, zero_prior=True, ties=True):
    """A root as a search could leave it: priors summing to one (one of them 0), visits on a few edges summing to N, several
    of them at n_max, W in [0, n]."""
    P = rng.random(M).astype(np.float32) + F32(1e-3)
    if zero_prior and M > 2:
        P[int(rng.integers(M))] = 0.0
    P = (P / P.sum(dtype=np.float32)).astype(np.float32)
    n = np.zeros(M, dtype=np.uint32)
    k = int(min(M, max(1, rng.integers(1, 17))))
    idx = rng.choice(M, size=k, replace=False)
    left = N
    top = max(1, N // k) if N else 0
    for i, j in enumerate(idx):
        take = min(left, top if (ties and i < 3) else int(rng.integers(0, top + 1)))
        n[j] = take
        left -= take
    W = (rng.random(M).astype(np.float32) * n.astype(np.float32)).astype(np.float32)
    W[n == 0] = 0.0
    return P, W, n


ROOT_CASES = [(M, N, v0) for M in (1, 2, 63, 64, 65, 128, 129, 200, 256)
              for N, v0 in ((0, 0.5), (1, 0.0), (16, 0.25), (33, 1.0), (100, 0.731))]


@pytest.mark.parametrize("M,N,v0", ROOT_CASES)
def test_root_equals_the_restatement(M, N, v0):
    rng = np.random.default_rng(1000 * M + N)
    P, W, n = _synthetic_root(rng, M, N)
    g = link.gumbel_noise(SEED, M, N, M)
    for c_visit, c_scale in ((50.0, 1.0), (0.0, 0.1), (16.0, 3.0)):
        move, counts = link.gumbel_root(P, W, n, v0, g, c_visit, c_scale)
        wmove, wcounts = gr.root(P, W, n, v0, g, c_visit, c_scale)
        assert move == wmove and (counts == wcounts).all(), (M, N, c_visit, c_scale)
        # the properties: the played edge has the most visits, the arg-max is written as 65535, nothing exceeds it
        assert n[move] == n.max() and counts.max() == 65535
        p = gr.improved_policy(P, W, n, v0, c_visit, c_scale)
        assert counts[int(np.argmax(p))] >= 65534
        assert (counts[P == 0] == 0).all()
        # the counts over their sum are the improved policy to the quantisation (each count is floor(65535 e_j): off by
        # less than one unit, and by the 2e-7 relative error of the f32 exponential and its argument, |x| < 100 here)
        e = p / p.max()
        assert (np.abs(counts.astype(np.float64) - 65535.0 * e) <= 1.0 + 65535.0 * e * 1e-4).all()


def test_root_has_unvisited_edges_zero_priors_and_ties_in_its_cases():
    seen_unvisited = seen_zero = seen_ties = 0
    for M, N, _ in ROOT_CASES:
        P, W, n = _synthetic_root(np.random.default_rng(1000 * M + N), M, N)
        seen_unvisited += int((n == 0).any() and N > 0)
        seen_zero += int((P == 0).any())
        seen_ties += int(N > 0 and (n == n.max()).sum() > 1)
    assert seen_unvisited > 10 and seen_zero > 10 and seen_ties > 10


def test_root_refuses_bad_arguments():
    P, W, n = _synthetic_root(np.random.default_rng(1), 8, 16)
    g = link.gumbel_noise(SEED, 0, 0, 8)
    for c_visit, c_scale in ((-1.0, 1.0), (float("nan"), 1.0), (50.0, 0.0), (50.0, float("inf")), (float("inf"), 1.0)):
        with pytest.raises(link.AzhError):
            link.gumbel_root(P, W, n, 0.5, g, c_visit, c_scale)
    with pytest.raises(ValueError):
        link.gumbel_root(P, W, n[:4], 0.5, g, 50.0, 1.0)
    with pytest.raises(link.AzhError):
        link.gumbel_root(P[:0], W[:0], n[:0], 0.5, g[:0], 50.0, 1.0)


@pytest.mark.parametrize("M,m,V", [(1, 4, 7), (3, 16, 16), (40, 4, 16), (40, 16, 33), (157, 256, 100), (200, 17, 100),
                                   (9, 8, 1), (64, 64, 64), (5, 2, 50)])
def test_a_simulated_search_never_lacks_a_candidate(M, m, V):
    """The root rule on a fresh root, simulation by simulation, with arbitrary scores: every simulation finds an edge with
    the schedule's visit count, and no more than min(m, M) edges are ever visited."""
    rng = np.random.default_rng(M * 1000 + m * 10 + V)
    P = rng.random(M).astype(np.float32)
    P = (P / P.sum(dtype=np.float32)).astype(np.float32)
    a = gr.a_values(P, link.gumbel_noise(SEED, M, V, M))
    n, W = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.float32)
    s = gr.seq(min(m, M), V)
    for t in range(V):
        j = gr.root_choice(a, W, n, s[t], 50.0, 1.0)
        assert j is not None, (t, s[t], n.tolist())
        n[j] += 1
        W[j] = F32(W[j] + F32(rng.random()))
    assert n.sum() == V and (n > 0).sum() <= min(m, M)
    # the first simulations go to the min(m, M) edges with the greatest a (the Gumbel-top-k trick), in that order
    k = min(m, M, V)
    order = np.argsort(-a.astype(np.float64), kind="stable")[:k]
    n2 = np.zeros(M, dtype=np.int64)
    for t in range(k):
        j = gr.root_choice(a, np.zeros(M, np.float32), n2, 0, 50.0, 1.0)
        assert j == order[t]
        n2[j] += 1


def test_a_nan_never_wins_and_equal_scores_go_to_the_lowest_index():
    a = np.array([0.5, np.nan, 0.5, 0.25], dtype=np.float32)
    n, W = [0, 0, 0, 0], [0.0] * 4
    assert gr.root_choice(a, W, n, 0, 50.0, 1.0) == 0
    assert gr.root_choice(a, W, [1, 0, 0, 0], 0, 50.0, 1.0) == 2
    assert gr.root_choice(a[1:2], W[:1], [0], 0, 50.0, 1.0) is None
    assert gr.root_choice(a, W, n, 3, 50.0, 1.0) is None
    # ... on the host as well: two equal best edges at n_max
    P = np.array([0.25, 0.25, 0.25, 0.25], dtype=np.float32)
    move, _ = link.gumbel_root(P, [1.0, 1.0, 0.0, 0.0], [2, 2, 0, 0], 0.5, np.zeros(4, np.float32), 50.0, 1.0)
    assert move == 0 and gr.root(P, [1.0, 1.0, 0.0, 0.0], [2, 2, 0, 0], 0.5, np.zeros(4, np.float32), 50.0, 1.0)[0] == 0
    move, _ = link.gumbel_root(P, [1.0, 1.5, 0.0, 0.0], [2, 2, 0, 0], 0.5, np.zeros(4, np.float32), 50.0, 1.0)
    assert move == 1
    move, _ = link.gumbel_root(P, [1.0, 1.5, 0.0, 0.0], [2, 2, 0, 0], 0.5, np.array([9, 0, 99, 0], np.float32), 0.0, 1.0)
    assert move == 0     # (the unvisited edge's noise does not count: it has not n_max visits)


def test_raising_an_edges_score_never_lowers_its_count():
    rng = np.random.default_rng(5)
    for M, N in ((8, 16), (65, 33), (200, 100)):
        P, W, n = _synthetic_root(rng, M, N, zero_prior=False)
        g = np.zeros(M, dtype=np.float32)
        for j in np.nonzero(n)[0][:4]:
            _, before = link.gumbel_root(P, W, n, 0.5, g, 50.0, 1.0)
            W2 = W.copy()
            W2[j] = min(F32(W[j] + F32(0.5)), F32(n[j]))
            _, after = link.gumbel_root(P, W2, n, 0.5, g, 50.0, 1.0)
            assert after[j] >= before[j], (M, j, before[j], after[j])
            # its share does not fall either
            assert after[j] / after.sum() >= before[j] / before.sum() - 1e-9


def test_a_vanishing_scale_gives_the_prior():
    rng = np.random.default_rng(9)
    for M, N in ((7, 16), (130, 100)):
        P, W, n = _synthetic_root(rng, M, N, zero_prior=True)
        _, counts = link.gumbel_root(P, W, n, 0.3, np.zeros(M, np.float32), 50.0, 1e-30)
        assert (counts == gr.root(P, W, n, 0.3, np.zeros(M, np.float32), 50.0, 1e-30)[1]).all()
        want = 65535.0 * P.astype(np.float64) / float(P.max())
        # floor(65535 exp(log P - log Pmax)): within one unit and the two logarithms' 2e-7 relative error each
        assert (np.abs(counts.astype(np.float64) - want) <= 1.0 + want * 1e-5).all()
        assert (counts[P == 0] == 0).all()


NAN, INF = float("nan"), float("inf")
DENORMAL = float(np.float32(1e-42))
# (name, prior, W, n, v0, c_visit, c_scale, the record is the move played alone)
HOSTILE_ROOTS = [
    ("all priors zero", [0, 0, 0, 0], [1.5, 0.5, 0, 0], [3, 1, 0, 0], 0.5, 50.0, 1.0, True),
    ("all priors zero, no visits", [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], 0.5, 50.0, 1.0, True),
    ("W NaN on the most visited edge", [.4, .3, .2, .1], [NAN, 0.5, 0, 0], [3, 1, 0, 0], 0.5, 50.0, 1.0, False),
    ("W NaN on every visited edge", [.4, .3, .2, .1], [NAN, NAN, 0, 0], [3, 3, 0, 0], 0.5, 50.0, 1.0, True),
    ("W NaN on every edge", [.4, .3, .2, .1], [NAN, NAN, NAN, NAN], [3, 3, 1, 1], 0.5, 50.0, 1.0, True),
    ("v0 NaN", [.4, .3, .2, .1], [1.5, 0.5, 0, 0], [3, 1, 0, 0], NAN, 50.0, 1.0, False),
    ("v0 NaN, no visits", [.4, .3, .2, .1], [0, 0, 0, 0], [0, 0, 0, 0], NAN, 50.0, 1.0, True),
    ("v0 +inf", [.4, .3, .2, .1], [1.5, 0.5, 0, 0], [3, 1, 0, 0], INF, 50.0, 1.0, True),
    ("v0 -inf", [.4, .3, .2, .1], [1.5, 0.5, 0, 0], [3, 1, 0, 0], -INF, 50.0, 1.0, False),
    ("W +inf", [.4, .3, .2, .1], [INF, 0.5, 0, 0], [3, 1, 0, 0], 0.5, 50.0, 1.0, True),
    ("W -inf", [.4, .3, .2, .1], [-INF, 0.5, 0, 0], [3, 1, 0, 0], 0.5, 50.0, 1.0, False),
    ("W +inf and -inf", [.4, .3, .2, .1], [INF, -INF, 0, 0], [3, 3, 0, 0], 0.5, 50.0, 1.0, True),
    ("no visits at all", [.4, .3, .2, .1], [0, 0, 0, 0], [0, 0, 0, 0], 0.5, 50.0, 1.0, False),
    ("one prior 1 and the rest 0", [0, 1, 0, 0], [0.5, 1.5, 0, 0], [1, 3, 0, 0], 0.5, 50.0, 1.0, False),
    ("one prior 1, the most visited edge another", [0, 1, 0, 0], [1.5, 0.5, 0, 0], [3, 1, 0, 0], 0.5, 50.0, 1.0, False),
    ("a denormal prior", [DENORMAL, .5, .5, 0], [1.5, 0.5, 0, 0], [3, 1, 0, 0], 0.5, 50.0, 1.0, False),
    ("every prior denormal (N / sum P overflows)", [DENORMAL] * 4, [1.5, 0.5, 0, 0], [3, 1, 0, 0], 0.5, 50.0, 1.0, True),
    ("ks overflows", [.4, .3, .2, .1], [1.5, 0.5, 0, 0], [3, 1, 0, 0], 0.5, 1e30, 1e30, True),
    ("ks overflows, no visits", [.4, .3, .2, .1], [0, 0, 0, 0], [0, 0, 0, 0], 0.5, 1e30, 1e30, True),
    ("one move, prior 0", [0], [0], [0], 0.5, 50.0, 1.0, True),
]


@pytest.mark.parametrize("case", HOSTILE_ROOTS, ids=[c[0] for c in HOSTILE_ROOTS])
def test_a_hostile_root_always_records_a_target(case):
    """Roots no benign evaluation leaves: the host equals the restatement, the played edge has the most visits, and some count
    is 65535 — where the improved policy has no finite greatest logit (x_max is -inf, +inf, or every x a NaN) the record is the
    move played with 65535 and nothing else, never an empty one."""
    name, P, W, n, v0, c_visit, c_scale, alone = case
    P, W, n = np.array(P, np.float32), np.array(W, np.float32), np.array(n, np.uint32)
    for g in (np.zeros(len(n), np.float32), link.gumbel_noise(SEED, 3, 5, len(n))):
        move, counts = link.gumbel_root(P, W, n, v0, g, c_visit, c_scale)
        wmove, wcounts = gr.root(P, W, n, v0, g, c_visit, c_scale)
        assert move == wmove and (counts == wcounts).all(), (name, move, wmove, counts, wcounts)
        assert n[move] == n.max()
        assert counts.max() == 65535, (name, counts)
        assert ((counts != 0).sum() == 1 and counts[move] == 65535) if alone else True, (name, counts)
        assert alone or (counts[P == 0] == 0).all()


def test_a_hostile_root_with_many_edges_and_the_move_beyond_the_first_lane_round():
    """200 edges, every prior 0, two edges at n_max: 70 with a finite W (its score is -inf, which does win) and 130 with a NaN
    one (which never does); with both NaN no score wins and the move is edge 0.  Either way the record is that move alone."""
    M = 200
    P, W, n = np.zeros(M, np.float32), np.zeros(M, np.float32), np.zeros(M, np.uint32)
    n[[70, 130]] = 5
    W[130] = NAN
    g = link.gumbel_noise(SEED, 1, 1, M)
    for W70, want in ((2.0, 70), (NAN, 0)):
        W[70] = W70
        move, counts = link.gumbel_root(P, W, n, 0.5, g, 50.0, 1.0)
        wmove, wcounts = gr.root(P, W, n, 0.5, g, 50.0, 1.0)
        assert move == wmove == want and (counts == wcounts).all()
        assert (counts != 0).sum() == 1 and counts[move] == 65535
    P[:] = 1.0 / M
    W[70] = 2.0
    move, counts = link.gumbel_root(P, W, n, 0.5, g, 50.0, 1.0)
    assert move == 70 == gr.root(P, W, n, 0.5, g, 50.0, 1.0)[0] and counts.max() == 65535 and counts[130] == 0


@pytest.mark.parametrize("beside", [["--eval-cache"], ["--forced-playouts", "2"], ["--fast-visits", "3"], ["--temperature", "1"],
                                    ["--root-policy-temperature", "1.25"], ["--one-random-move"]])
def test_the_generator_refuses_what_does_not_go_with_gumbel_actions(tmp_path, beside):
    """an explicit --eval-cache or a refused mode beside --gumbel-actions ends the generator with a message before it touches
    a device or its files"""
    games_path = str(tmp_path / "model-004-0.json")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "accelerated_generate_games.py"), "--network",
                          str(tmp_path / "none.npy"), "--output-games", games_path, "--visits", "6", "--gumbel-actions", "4"]
                         + beside, cwd=ROOT, capture_output=True, timeout=120)
    assert res.returncode != 0 and b"--gumbel-actions does not go with " + beside[0].encode() in res.stderr
    assert not os.path.exists(games_path)


@pytest.mark.parametrize("bad", [["--gumbel-actions", "257"], ["--gumbel-actions", "4", "--gumbel-c-scale", "0"],
                                 ["--gumbel-actions", "4", "--gumbel-c-visit", "-1"],
                                 ["--gumbel-actions", "256", "--visits", "4097"]])
def test_the_generator_refuses_gumbel_parameters_out_of_range(tmp_path, bad):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "accelerated_generate_games.py"), "--network",
                          str(tmp_path / "none.npy"), "--output-games", str(tmp_path / "g-0.json")] + bad,
                         cwd=ROOT, capture_output=True, timeout=120)
    assert res.returncode != 0 and b"--gumbel-actions needs 1 <= M <= 256" in res.stderr
