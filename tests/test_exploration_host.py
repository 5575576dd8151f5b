"""First-play urgency and the growing exploration rate without a device: the library's host export
(azh_exploration_scores — the functions the leaf-parallel kernel's level uses, the two 64-lane sums restated lane by lane)
against tests/exploration_reference.py, bit for bit."""
import numpy as np
import pytest

from ataxxzero_amd import link
from tests import exploration_reference as xr
from tests import priors_reference as pr
from tests import vl_reference as vlr

F32 = np.float32
SIZES = [1, 2, 63, 64, 65, 128, 129, 200, 255]
PARAMS = [(0.25, 0.0, 0.0), (-1.0, 19652.0, 1.25), (0.25, 19652.0, 1.25), (0.0, 1.0, 3.0), (1.5, 0.5, 0.0)]


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _same(got, want):
    """bit for bit, a NaN being a NaN on both sides (which NaN an operation hands on is the hardware's choice)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    assert got.shape == want.shape and (np.isnan(got) == nan).all()
    assert (_bits(got)[~nan] == _bits(want)[~nan]).all()


def _node(rng, M, visited=0.6):
    """random priors (a softmax), visits (some edges unvisited) and total scores W in [0, n]"""
    x = rng.standard_normal(M).astype(np.float32)
    prior = (np.exp(x) / np.exp(x).sum()).astype(np.float32)
    n = (rng.integers(1, 400, size=M) * (rng.random(M) < visited)).astype(np.uint32)
    W = (rng.random(M).astype(np.float32) * n.astype(np.float32)).astype(np.float32)
    return prior, W, n


def _both(prior, W, n, c_puct, r, c_base, c_init):
    got = link.exploration_scores(prior, W, n, c_puct, r, c_base, c_init)
    want = xr.scores(prior, W, n, int(n.astype(np.uint64).sum()), c_puct, r, c_base, c_init)
    _same(got, want)
    return got


@pytest.mark.parametrize("M", SIZES)
def test_random_nodes_equal_the_restatement(M):
    rng = np.random.default_rng(1000 + M)
    for params in PARAMS:
        for c_puct in (1.0, 2.5):
            for visited in (0.1, 0.6, 1.0):
                _both(*_node(rng, M, visited), c_puct, *params)


@pytest.mark.parametrize("M", SIZES)
def test_nodes_without_a_visit_score_in_the_priors_order(M):
    rng = np.random.default_rng(2000 + M)
    prior, W, n = _node(rng, M, visited=0.0)
    assert n.sum() == 0
    for params in PARAMS:
        sc = _both(prior, W, n, 1.0, *params)
        # f = 0 (N == 0): the scores are c * P, so their order is the priors' order
        c = xr.rate(0, 1.0, params[1], params[2])
        _same(sc, np.array([F32(F32(1.0) / F32(1.0)) * (c * p) + F32(0.0) for p in prior], dtype=np.float32))
        assert (np.argsort(-sc, kind="stable") == np.argsort(-prior, kind="stable")).all()
        assert vlr.pick(sc, True) == int(np.argmax(prior))


@pytest.mark.parametrize("M", [3, 65, 200])
def test_non_finite_total_scores(M):
    rng = np.random.default_rng(3000 + M)
    for bad in ([np.nan], [np.inf], [-np.inf], [np.inf, -np.inf], [np.nan, np.inf]):
        prior, W, n = _node(rng, M, visited=0.7)
        n[0] = 0                        # an unvisited edge, whose score is U + f
        for i, v in enumerate(bad):
            n[1 + i] = 5
            W[1 + i] = v
        if M > 64:                      # one beyond the first round of lanes too
            n[64], W[64] = 3, bad[0]
        for params in PARAMS:
            sc = _both(prior, W, n, 1.0, *params)
            N = int(n.sum())
            f = xr.fpu(prior, W, n, N, params[0])
            assert not np.isnan(f) and f >= 0
            if np.isnan(bad).any() or (np.inf in bad and -np.inf in bad) or bad == [-np.inf]:
                assert f == 0           # a NaN or a negative mean: the floor
            # a NaN score is never picked, whatever the tie rule
            for tie_first in (False, True):
                assert not np.isnan(sc[vlr.pick(sc, tie_first)])


@pytest.mark.parametrize("M", SIZES)
def test_the_mode_off_is_the_reference_puct(M):
    rng = np.random.default_rng(4000 + M)
    for c_puct in (1.0, 0.7):
        prior, W, n = _node(rng, M)
        got = link.exploration_scores(prior, W, n, c_puct, *xr.OFF)
        want = vlr.puct_scores(prior, W, n, int(n.sum()), c_puct)
        assert (_bits(got) == _bits(want)).all()
        assert (_bits(xr.scores(prior, W, n, int(n.sum()), c_puct, *xr.OFF)) == _bits(want)).all()
        assert (_bits(link.exploration_scores(prior, W, n, c_puct)) == _bits(want)).all()      # (the defaults are "off")
        # c_init alone switches nothing on
        assert (_bits(link.exploration_scores(prior, W, n, c_puct, -1.0, 0.0, 7.0)) == _bits(want)).all()


def test_the_sums_are_in_lane_order_not_in_index_order():
    t = F32(2.0 ** -24)
    # terms 1 and 65 meet in lane 1 (2^-23, which 1 can hold) before lane 1 meets lane 0; one after the other each is lost
    M = 66
    W = np.zeros(M, dtype=np.float32)
    W[0], W[1], W[65] = 1.0, t, t
    seq = F32(0.0)
    for x in W:
        seq = F32(seq + x)
    assert seq == F32(1.0) and pr.wave_sum(W) == F32(1.0 + 2.0 ** -23)
    prior = np.zeros(M, dtype=np.float32)
    prior[0] = 1.0
    n = np.zeros(M, dtype=np.uint32)
    n[0] = 1                            # N = 1: qX = Wsum; r = 0: f = qX; prior 0: an unvisited edge scores f itself
    sc = _both(prior, W, n, 1.0, 0.0, 0.0, 0.0)
    assert sc[2] == pr.wave_sum(W) and sc[2] != seq
    # the policy mass likewise: P over the visited children, summed in lane order, under the square root
    # (a mass of 2.25 — no policy, but arithmetic all the same: its root is 1.5 exactly, and one ulp more shows under the root)
    t = F32(2.0 ** -23)
    prior = np.zeros(M, dtype=np.float32)
    prior[0], prior[1], prior[65] = 2.25, t, t
    seq = F32(0.0)
    for x in prior:
        seq = F32(seq + x)
    assert seq == F32(2.25) and pr.wave_sum(prior) == F32(2.25 + 2.0 ** -22)
    n = np.ones(M, dtype=np.uint32)
    W = np.full(M, 1.0, dtype=np.float32)
    n[2], W[2], prior[2] = 0, 0.0, 0.0
    sc = _both(prior, W, n, 1.0, 0.5, 0.0, 0.0)
    with_lanes = F32(F32(pr.wave_sum(W) / F32(65)) - F32(F32(0.5) * np.sqrt(pr.wave_sum(prior))))
    in_index_order = F32(F32(pr.wave_sum(W) / F32(65)) - F32(F32(0.5) * np.sqrt(seq)))
    assert sc[2] == with_lanes and with_lanes != in_index_order


def _pick(params, c_puct=1.0):
    """the edge picked at the node of the knob test: child 0 visited (P 0.9, n 10, W 8), child 1 unvisited (P 0.1) — by the
    library's scores, which equal the restatement's"""
    prior = np.array([0.9, 0.1], dtype=np.float32)
    W = np.array([8.0, 0.0], dtype=np.float32)
    n = np.array([10, 0], dtype=np.uint32)
    sc = _both(prior, W, n, c_puct, *params)
    assert vlr.pick(sc, True) == vlr.pick(xr.scores(prior, W, n, 10, c_puct, *params), True)
    return vlr.pick(sc, True), sc


def test_the_knobs_are_wired():
    visited, unvisited = 0, 1
    off, sc_off = _pick(xr.OFF)
    assert off == visited                               # an unvisited move is a loss: 0.33 against 1.07
    assert _pick((0.0, 0.0, 0.0))[0] == unvisited       # f = 0.8, the node's mean score
    assert _pick((0.5, 0.0, 0.0))[0] == visited         # f = 0.8 - 0.5 sqrt(0.9)
    # The rate, FPU off.  At this node the visited child leads while c < 0.8 / (sq (0.1 - 0.9 / 11)) = 13.27 (sq = sqrt(11));
    # c_base = 1, c_init = 3 give c = log(12) + 3 = 5.48, which moves every score and leaves the pick, and c_init = 11 gives
    # 13.48, which changes it.
    same, sc = _pick((-1.0, 1.0, 3.0))
    assert same == visited and (sc > sc_off).all()
    assert xr.rate(10, 1.0, 1.0, 3.0) == F32(xr.logf(F32(12.0)) + F32(3.0))
    assert _pick((-1.0, 1.0, 11.0))[0] == unvisited


def test_refusals_of_the_host_call():
    prior, W, n = _node(np.random.default_rng(5), 7)
    for bad in [(np.nan, 0, 0), (0.25, np.nan, 0), (0.25, 1.0, np.nan), (np.inf, 0, 0), (-np.inf, 0, 0), (0.25, np.inf, 0),
                (0.25, 1.0, np.inf), (0.25, -1.0, 0), (0.25, 1.0, -0.5)]:
        with pytest.raises(link.AzhError) as ei:
            link.exploration_scores(prior, W, n, 1.0, *bad)
        assert str(ei.value) == ("ataxxzero_hip error -2: azh_exploration_scores: need finite arguments, c_base >= 0 and "
                                 "c_init >= 0")
    for M in (0, 257):
        with pytest.raises(link.AzhError) as ei:
            link.exploration_scores(np.zeros(M, np.float32), np.zeros(M, np.float32), np.zeros(M, np.uint32), 1.0)
        assert str(ei.value).startswith("ataxxzero_hip error -1: azh_exploration_scores: bad argument")
    with pytest.raises(ValueError):
        link.exploration_scores(prior, W[:3], n, 1.0)
